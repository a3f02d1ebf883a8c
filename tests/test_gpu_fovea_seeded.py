"""The seeded (warm) foveated call on the device: ugsm_stage_warm_stack, ugsm_submit_foveated_warm[_field], ugsm_match_foveated_warm.

The definition (include/ugsm.h): the starting field of fovea level k is the crop, at the new window's origin, of the restriction to level k of
the full-resolution field ugsm_reconstruct_full gives for the prior stack; level start_level is matched from its starting field, never as a top
level, the levels below follow as the fine phase of ugsm_submit_foveated runs them, and the row blocks above start_level receive their starting
fields.  tests/fovea_seeded_np.py composes exactly that of the CPU oracle's stages; every comparison here is equality of float32 bit patterns
(NaN where NaN).  The priors are other pairs' cold stacks at other offsets, and every definition test asserts its premise from the oracle
alone: the wanted stack differs from the pair's cold stack, so a call that ignores its prior cannot pass."""
import numpy as np
import pytest

import encode_np as en
import fovea_seeded_np as fs
import launch_census as lc
import seeded_np as sn
from conftest import assert_bit_equal
from test_gpu_input_format import Dev

pytestmark = pytest.mark.gpu

W, H, LEVELS, F = lc.W, lc.H, lc.LEVELS, lc.F          # 333 x 251: every one of the 14 levels exists
STARTS = (0, 1, 4, 5, 6)
NEW = lc.OFFS3                                          # pair j's new window: centred, off-centre, clamped into a corner
PRIOR_OF = [(j + 1) % 3 for j in range(3)]              # pair j's prior: pair (j + 1) % 3's cold stack, matched at that pair's own offsets


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


# ---- the oracle's answers, computed once and shared, never written to --------------------------------------------------------------------

_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
        _MEMO[key] = v
    return _MEMO[key]


def _cold(orc, j, off=None):
    off = NEW[j] if off is None else off
    return _memo(("cold", j, off), lambda: orc.match_foveated(*lc.pairs()[j], LEVELS, F, off[0], off[1])[0])


def _pyr(orc, j):
    return _memo(("pyr", j), lambda: tuple(a for side in sn.pyramids(orc, *lc.pairs()[j], LEVELS) for a in side))


def _prior(orc, j):
    return _cold(orc, PRIOR_OF[j]), NEW[PRIOR_OF[j]]


def _warm(orc, j, s, prior=None, poff=None, off=None, key=None):
    def make():
        p = _pyr(orc, j)
        pr, po = _prior(orc, j) if prior is None else (prior, poff)
        return fs.warm_oracle(orc, None, None, pr, LEVELS, po, NEW[j] if off is None else off, s, (p[:LEVELS], p[LEVELS:]))
    return _memo(("warm", j, s, key), make)


def _premise(orc, j, s, want, off=None):
    cold = _cold(orc, j, off)
    assert not np.array_equal(want.view(np.uint32), cold.view(np.uint32)), f"premise: pair {j} warm from level {s} equals its cold stack"
    assert not np.array_equal(want[:, :s + 1].view(np.uint32), cold[:, :s + 1].view(np.uint32)), f"premise: pair {j}, the matched levels 0 .. {s}"


def _context(lib, policy, **kw):
    cfg, env = lc.POLICIES[policy]
    with lc._environ(env):
        return lib.Context(levels=kw.pop("levels", LEVELS), fovea_levels=kw.pop("fovea_levels", F), **dict(cfg, **kw))


def _stack_floats(lib, w=W, h=H, levels=LEVELS, F_=F):
    fw, fh = lib.fovea_dims(w, h, levels, F_)
    return 3 * F_ * fh * fw, (3, F_, fh, fw)


def _submit(c, lib, pairs, priors, poffs, offs, s, slot=0, field=False):
    """One warm call of host images and host priors into NaN-filled stacks; the stacks back."""
    d = Dev(c)
    try:
        put = [(d.put(L)[0], d.put(R)[0]) for L, R in pairs]
        stride = pairs[0][0].strides[0]
        dP = [c.to_device(np.ascontiguousarray(p, np.float32)) for p in priors]
        d.bufs += dP
        nf, shape = _stack_floats(lib)
        dO = [d.out(nf) for _ in pairs]
        if field:
            c.submit_foveated_warm_field(slot, [p[0] for p in put], [p[1] for p in put], W, H, stride, offs, dP, s, dO)
        else:
            c.submit_foveated_warm(slot, [p[0] for p in put], [p[1] for p in put], W, H, stride, offs, dP, poffs, s, dO)
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return [c.to_host(p, shape) for p in dO]
    finally:
        d.free()


# ---- 1. the starting-field launch against the device's own composition, and against numpy -------------------------------------------------

def _device_composition(c, lib, orc, prior, w, h, levels, poff, off, s):
    """ugsm_reconstruct_full -> ugsm_stage_restrict -> a numpy crop, for the levels s .. F-1."""
    F_ = prior.shape[1]
    lw, lh = lib.level_dims(w, h, levels)
    fw, fh, ox, oy, _, _ = fs.origins(orc, w, h, levels, F_, off)
    planes = [c.to_device(np.ascontiguousarray(prior[p])) for p in range(3)]
    full, lvl = c.alloc(4 * 3 * w * h), c.alloc(4 * 3 * w * h)
    try:
        c.reconstruct_full(planes[0], planes[1], planes[2], w, h, full, poff[0], poff[1])
        out = {}
        for k in range(s, F_):
            c.stage_restrict(full, w, h, k, lvl)
            out[k] = c.to_host(lvl, (3, lh[k], lw[k]))[:, oy[k]:oy[k] + fh, ox[k]:ox[k] + fw]
        return out
    finally:
        for p in planes + [full, lvl]:
            c.free(p)


STAGE_CASES = [
    (333, 251, 14, 7, (0, 0), lc.OFF_CENTRE),            # prior centred -> new off-centre
    (333, 251, 14, 7, (5000, -5000), (0, 0)),            # prior in a corner -> new centred
    (333, 251, 14, 7, lc.OFF_CENTRE, lc.OFF_CENTRE),     # prior and new equal
    (67, 49, 9, 2, (0, 0), (9, -7)),
    (333, 251, 14, 14, (0, 0), lc.OFF_CENTRE),           # F = levels
]


@pytest.mark.parametrize("w,h,levels,F_,poff,off", STAGE_CASES, ids=["centred-to-off-centre", "corner-to-centred", "equal", "67x49-nine-levels-F2", "F-is-levels"])
def test_stage_warm_stack_against_the_device_composition_and_numpy(lib, orc, w, h, levels, F_, poff, off):
    nf, shape = _stack_floats(lib, w, h, levels, F_)
    prior = fs.special_stack(F_, shape[2], shape[3], 5100 + w + F_)
    with lib.Context(levels=levels, fovea_levels=F_) as c:
        fill = np.full(nf + 64, np.nan, np.float32)      # (stays referenced while the copies read it)
        src, dst = c.to_device(prior), c.to_device(fill)
        try:
            device = _device_composition(c, lib, orc, prior, w, h, levels, poff, off, 0)
            want = fs.start_fields(orc, prior, w, h, levels, poff, off, 0)
            for s in range(F_):
                c.check(c.lib.ugsm_copy_to_device(c.handle, dst, fill.ctypes.data, fill.nbytes))
                c.stage_warm_stack(src, w, h, poff, off, s, dst)
                raw = c.to_host(dst, (nf + 64,))
                got = raw[:nf].reshape(shape)
                for k in range(s, F_):
                    assert_bit_equal(got[:, k], device[k], f"{w}x{h} F = {F_}, start level {s}, level {k}: against reconstruct -> restrict -> crop on the device")
                    assert_bit_equal(got[:, k], want[k], f"{w}x{h} F = {F_}, start level {s}, level {k}: against numpy")
                assert np.isnan(got[:, :s]).all(), f"start level {s}: a row block below it was written"
                assert np.isnan(raw[nf:]).all(), f"start level {s}: written past the stack"
            for bad in (F_, -1):
                assert c.lib.ugsm_stage_warm_stack(c.handle, src, w, h, 0, 0, 0, 0, bad, dst) == lib.UGSM_ERR_BAD_ARG
            assert c.lib.ugsm_stage_warm_stack(c.handle, None, w, h, 0, 0, 0, 0, 0, dst) == lib.UGSM_ERR_BAD_ARG
            assert c.lib.ugsm_stage_warm_stack(c.handle, src, w, h, 0, 0, 0, 0, 0, src) == lib.UGSM_ERR_BAD_ARG
        finally:
            c.free(src)
            c.free(dst)


# ---- 2. the call against the oracle --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("s", STARTS)
@pytest.mark.parametrize("policy", list(lc.POLICIES))
def test_definition(lib, orc, policy, s, n):
    js = list(range(n))
    want = [_warm(orc, j, s) for j in js]
    for j in js:
        _premise(orc, j, s, want[j])
    if n == 3:
        assert len({_prior(orc, j)[0].tobytes() for j in js}) == 3 and len({_prior(orc, j)[1] for j in js}) == 3, "premise: three priors at three offsets"
    with _context(lib, policy, batch=n) as c:
        outs = _submit(c, lib, [lc.pairs()[j] for j in js], [_prior(orc, j)[0] for j in js], [_prior(orc, j)[1] for j in js], [NEW[j] for j in js], s)
    for j in js:
        moved = np.nanmean(np.abs(want[j][:2, :s + 1].astype(np.float64) - _cold(orc, j)[:2, :s + 1]))
        print(f"{policy}, start level {s}, pair {j} of {n}: oracle warm vs cold mean |d| over the matched levels = {moved:.3f} px")
        assert_bit_equal(outs[j], want[j], f"{policy}, start level {s}, pair {j} of {n}")


# ---- 3. the field form ---------------------------------------------------------------------------------------------------------------------

def test_a_full_resolution_field_as_the_prior(lib, orc):
    s, j = 5, 0
    field = _memo(("full", 2), lambda: orc.match_full(*lc.pairs()[2], LEVELS))
    p = _pyr(orc, j)
    want = fs.warm_oracle(orc, None, None, field, LEVELS, None, lc.OFF_CENTRE, s, (p[:LEVELS], p[LEVELS:]), field=True, F=F)
    _premise(orc, j, s, want, lc.OFF_CENTRE)
    with lib.Context(levels=LEVELS, fovea_levels=F) as c:
        got = _submit(c, lib, [lc.pairs()[j]], [field], None, [lc.OFF_CENTRE], s, field=True)[0]
    assert_bit_equal(got, want, "the field form, start level 5: restrict -> crop -> descent")


# ---- 4. bgr8 -------------------------------------------------------------------------------------------------------------------------------

def test_bgr8(lib, orc):
    s, (L, R) = 4, lc.pairs()[0]
    want = _warm(orc, 0, s)
    _premise(orc, 0, s, want)
    a, b = en.encode(L, en.BGR8), en.encode(R, en.BGR8)
    assert np.array_equal(en.to_rgb8(a, en.BGR8), L) and not np.array_equal(a, L)
    with lib.Context(levels=LEVELS, fovea_levels=F) as c:
        c.set_input_format(en.BGR8)
        out = _submit(c, lib, [(a, b)], [_prior(orc, 0)[0]], [_prior(orc, 0)[1]], [NEW[0]], s)[0]
        assert c.input_format == en.BGR8
    assert_bit_equal(out, want, "bgr8 images, start level 4")


# ---- 5. kernel_path 1 ----------------------------------------------------------------------------------------------------------------------

def test_kernel_path_1_runs_the_pairs_one_after_the_other(lib, orc):
    """libugsm_dev.so, one kernel per reference stage: the same stacks as the default path (and so the oracle's)."""
    s = 5
    pairs, priors, poffs = lc.pairs(), [_prior(orc, j)[0] for j in range(3)], [_prior(orc, j)[1] for j in range(3)]
    with lib.Context(levels=LEVELS, fovea_levels=F, batch=3) as c:
        default = _submit(c, lib, pairs, priors, poffs, NEW, s)
    with lib.Context(levels=LEVELS, fovea_levels=F, kernel_path=1, dev=True, profile_events=2) as c:
        dev = _submit(c, lib, pairs, priors, poffs, NEW, s)
        launches = sum(st["launches"] for st in c.kernel_stats() if st["name"] == "k_restrict_stack")
    assert launches == 3, "pair by pair: one starting-field launch per pair"
    for j in range(3):
        _premise(orc, j, s, _warm(orc, j, s))
        assert_bit_equal(dev[j], default[j], f"kernel_path 1 against the default path, pair {j}")
        assert_bit_equal(dev[j], _warm(orc, j, s), f"kernel_path 1 against the oracle, pair {j}")


# ---- 6. chaining ---------------------------------------------------------------------------------------------------------------------------

def test_two_calls_back_to_back_alternating_two_stacks(lib, orc):
    """Frame after frame on one slot, no wait in between: the window moves, the second call's prior is the first's d_stack."""
    s1, s2, at1, at2 = 5, 4, NEW[0], (NEW[0][0] + 9, NEW[0][1] - 6)
    f1 = _warm(orc, 0, s1)
    f2 = _warm(orc, 2, s2, prior=f1, poff=at1, off=at2, key="chain")
    _premise(orc, 2, s2, f2, at2)
    other = _warm(orc, 2, s2, prior=_prior(orc, 0)[0], poff=_prior(orc, 0)[1], off=at2, key="chain-from-the-first-prior")
    assert not np.array_equal(f2.view(np.uint32), other.view(np.uint32)), "premise: the chain's prior matters"
    nf, shape = _stack_floats(lib)
    with lib.Context(levels=LEVELS, fovea_levels=F) as c:
        d = Dev(c)
        try:
            (l0, stride), (r0, _), (l2, _), (r2, _) = [d.put(a) for a in lc.pairs()[0] + lc.pairs()[2]]
            prior = c.to_device(_prior(orc, 0)[0])
            d.bufs.append(prior)
            a, b = d.out(nf), d.out(nf)
            c.submit_foveated_warm(0, [l0], [r0], W, H, stride, [at1], [prior], [_prior(orc, 0)[1]], s1, [a])
            c.submit_foveated_warm(0, [l2], [r2], W, H, stride, [at2], [a], [at1], s2, [b])
            c.check(c.lib.ugsm_wait(c.handle, 0))
            got1, got2 = c.to_host(a, shape), c.to_host(b, shape)
        finally:
            d.free()
    assert_bit_equal(got1, f1, "the first of two chained calls")
    assert_bit_equal(got2, f2, "the second of two chained calls, from the first's stack, the window moved")


def test_nine_calls_of_three_pairs_back_to_back_take_turns_on_the_upload_ring(lib, orc):
    """Three pairs are more than travel in the starting-field launch's arguments: their rows go up through the slot's table, from page-locked
    copies that take turns.  Nine calls on one slot with no wait between them, each into stacks of its own, rotating through three sets of
    window offsets, so that call k and call k - 4 -- which fill the same copy -- never share a table: a stale copy shows as a wrong stack.
    From start level 0 (the shortest call).  Every stack is bit-equal to the same call made alone and waited for on that context."""
    s, pairs = min(STARTS), lc.pairs()
    priors, poffs = [_prior(orc, j)[0] for j in range(3)], [_prior(orc, j)[1] for j in range(3)]
    sets = [[NEW[(j + r) % 3] for j in range(3)] for r in range(3)]
    assert all(sets[k % 3] != sets[(k - 4) % 3] for k in range(4, 9))
    nf, shape = _stack_floats(lib)
    with lib.Context(levels=LEVELS, fovea_levels=F, batch=3) as c:
        d = Dev(c)
        try:
            put = [(d.put(L)[0], d.put(R)[0]) for L, R in pairs]
            stride = pairs[0][0].strides[0]
            dP = [c.to_device(np.ascontiguousarray(p, np.float32)) for p in priors]
            d.bufs += dP

            def call(offs):
                dO = [d.out(nf) for _ in pairs]
                c.submit_foveated_warm(0, [p[0] for p in put], [p[1] for p in put], W, H, stride, offs, dP, poffs, s, dO)
                return dO
            alone = []
            for offs in sets:
                dO = call(offs)
                c.check(c.lib.ugsm_wait(c.handle, 0))
                alone.append([c.to_host(p, shape) for p in dO])
            for j in range(3):    # the premise: the three sets give pair j three different stacks
                assert len({alone[r][j].tobytes() for r in range(3)}) == 3, f"premise: pair {j}"
            assert_bit_equal(alone[0][0], _warm(orc, 0, s), "the call made alone, against the oracle")
            queued = [call(sets[k % 3]) for k in range(9)]
            c.check(c.lib.ugsm_wait(c.handle, 0))
            for k in range(9):
                for j in range(3):
                    assert_bit_equal(c.to_host(queued[k][j], shape), alone[k % 3][j], f"call {k} of nine back to back, pair {j}")
        finally:
            d.free()


# ---- 7. what runs --------------------------------------------------------------------------------------------------------------------------

def _is_level_work(name):
    return name.startswith(("k_cost", "k_smooth", "k_sqblur", "k_seed", "k_box", "k_warp"))


def _is_pyramid(name):
    return name.startswith(("k_pyr", "k_blur_decimate"))


@pytest.mark.parametrize("n", [1, 3])
def test_census_at_start_level_4(lib, orc, n):
    s = 4
    fw, fh = lib.fovea_dims(W, H, LEVELS, F)
    js = list(range(n))
    pairs, priors, poffs, offs = [lc.pairs()[j] for j in js], [_prior(orc, j)[0] for j in js], [_prior(orc, j)[1] for j in js], [NEW[j] for j in js]
    with lib.Context(levels=LEVELS, fovea_levels=F, slots=1, profile_events=2, batch=n) as c:
        outs = _submit(c, lib, pairs, priors, poffs, offs, s)
        stats = [st for st in c.kernel_stats() if st["launches"] > 0]
    with lib.Context(levels=LEVELS, fovea_levels=F, slots=1, profile_events=2, batch=n) as c:       # the yardstick: the plain call, same pairs, same context
        d = Dev(c)
        put = [(d.put(L)[0], d.put(R)[0]) for L, R in pairs]
        c.submit_foveated_batch(0, [p[0] for p in put], [p[1] for p in put], W, H, pairs[0][0].strides[0], offs, [d.out(_stack_floats(lib)[0]) for _ in js])
        c.check(c.lib.ugsm_wait(c.handle, 0))
        plain = [st for st in c.kernel_stats() if st["launches"] > 0]
        d.free()
    for j in js:
        assert_bit_equal(outs[j], _warm(orc, j, s), f"profiled call, pair {j}")
    above = [(st["name"], st["level"]) for st in stats if s < st["level"] < LEVELS and _is_level_work(st["name"])]
    assert not above, f"level work above level {s}: {above}"
    pyr_above = [(st["name"], st["level"]) for st in stats if max(s, 2) < st["level"] < LEVELS and _is_pyramid(st["name"])]
    assert not pyr_above, f"pyramid launches above level {max(s, 2)}: {pyr_above}"
    start = [st for st in stats if st["name"] == "k_restrict_stack"]
    assert [(st["level"], st["launches"], st["pixel_launches"]) for st in start] == [(s, 1, float(n * (F - s) * fw * fh))], start

    def counts(rows, prefix):
        return {lv: sum(st["launches"] for st in rows if st["name"].startswith(prefix) and st["level"] == lv) for lv in range(s + 1)}
    for prefix in ("k_cost", "k_smooth"):
        assert counts(stats, prefix) == counts(plain, prefix), prefix
        assert all(v > 0 for v in counts(stats, prefix).values()), prefix
    assert sum(st["launches"] for st in stats) < sum(st["launches"] for st in plain)


# ---- 8. the blocking call ------------------------------------------------------------------------------------------------------------------

def test_match_foveated_warm_from_pageable_memory(lib, orc):
    s, j = 4, 1
    L, R = lc.pairs()[j]
    want = _warm(orc, j, s)
    _premise(orc, j, s, want)
    prior, poff = np.array(_prior(orc, j)[0]), _prior(orc, j)[1]        # pageable, writable: the call must leave it alone
    keep = prior.copy()
    at2 = (NEW[j][0] + 7, NEW[j][1] + 5)
    with lib.Context(levels=LEVELS, fovea_levels=F) as c:
        got = c.match_foveated_warm(L, R, prior, poff, NEW[j], s)
        again = c.match_foveated_warm(L, R, got, NEW[j], at2, 0)        # ... and a second frame from the first's result, the window moved
    assert_bit_equal(prior, keep, "the prior after the call")
    assert_bit_equal(got, want, "ugsm_match_foveated_warm, start level 4")
    assert_bit_equal(again, _warm(orc, j, 0, prior=want, poff=NEW[j], off=at2, key="again"), "ugsm_match_foveated_warm from its own result, start level 0")
    from ug_stereomatcher_amd import MatchGPULib
    m = MatchGPULib(levels=LEVELS)
    try:
        assert m.getFoveateLevel() == F
        got_m = m.matchStackSeeded(L, R, np.ascontiguousarray(prior.transpose(1, 0, 2, 3)), poff, NEW[j], s)
        assert_bit_equal(got_m, want.transpose(1, 0, 2, 3), "MatchGPULib.matchStackSeeded")
    finally:
        m.close()


# ---- 9. refusals on the device -------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device_write_nothing(lib, orc):
    L, R = lc.pairs()[0]
    nf, shape = _stack_floats(lib)
    with lib.Context(levels=LEVELS, fovea_levels=F) as c:
        d = Dev(c)
        try:
            (pl, stride), (pr, _) = d.put(L), d.put(R)
            fill = np.full(nf, np.nan, np.float32)               # (stays referenced while the copies read it)
            a, b = c.to_device(fill), c.to_device(fill)
            d.bufs += [a, b]
            with pytest.raises(lib.UgsmError) as e:
                c.submit_foveated_warm(0, [pl], [pr], W, H, stride, None, [a], None, 3, [a])
            assert e.value.status == lib.UGSM_ERR_BAD_ARG
            c.set_lr_check(1.0, lib.UGSM_LR_FOVEATED)
            with pytest.raises(lib.UgsmError) as e:
                c.submit_foveated_warm(0, [pl], [pr], W, H, stride, None, [a], None, 3, [b])
            assert e.value.status == lib.UGSM_ERR_STATE
            c.set_lr_check(0.0, 0)
            for bad in (F, -1):
                with pytest.raises(lib.UgsmError) as e:
                    c.submit_foveated_warm(0, [pl], [pr], W, H, stride, None, [a], None, bad, [b])
                assert e.value.status == lib.UGSM_ERR_BAD_ARG
            c.check(c.lib.ugsm_wait(c.handle, 0))
            for p in (a, b):
                assert np.isnan(c.to_host(p, (nf,))).all(), "a refused call wrote nothing"
        finally:
            d.free()
