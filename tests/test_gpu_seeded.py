"""The seeded full-mode call on the device: ugsm_stage_restrict, ugsm_submit_full_seeded, ugsm_match_full_seeded.

The definition (include/ugsm.h): d_out[k] is the field reached by restricting d_prior[k] to level start_level, running matchlevel on the
levels start_level .. 0 with subsampleDisp between them, and never taking the top level's first-iteration exception.  tests/seeded_np.py
composes exactly that of the CPU oracle's stages and a numpy restriction written from the definition; every comparison here is equality of
float32 bit patterns (NaN where NaN).  The priors are other pairs' cold results -- the use case -- and every definition test asserts its
premise from the oracle alone: the seeded field differs from the cold one, so a call that ignores its prior cannot pass."""
import numpy as np
import pytest

import encode_np as en
import launch_census as lc
import seeded_np as sn
from conftest import assert_bit_equal
from test_gpu_input_format import Dev

pytestmark = pytest.mark.gpu

W, H, LEVELS = lc.W, lc.H, lc.LEVELS          # 333 x 251: every one of the 14 levels exists
STARTS = (0, 1, 4, 5, 13)


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


def _cold(orc, j):
    return _memo(("cold", j), lambda: orc.match_full(*lc.pairs()[j], LEVELS))


def _pyr(orc, j):
    return _memo(("pyr", j), lambda: tuple(a for side in sn.pyramids(orc, *lc.pairs()[j], LEVELS) for a in side))


def _prior(orc, j):
    """Pair j's prior: another pair's cold result (pair 1 is the one with the zero patch in its left image)."""
    return _cold(orc, (j + 1) % 3)


def _seeded(orc, j, s, prior=None, key=None):
    def make():
        p = _pyr(orc, j)
        return sn.seeded_oracle(orc, None, None, _prior(orc, j) if prior is None else prior, s, LEVELS, (p[:LEVELS], p[LEVELS:]))
    return _memo(("seeded", j, s, key), make)


def _premise(orc, j, s, seeded):
    cold = _cold(orc, j)
    assert not np.array_equal(seeded.view(np.uint32), cold.view(np.uint32)), f"premise: pair {j} seeded at level {s} equals its cold field"


def _context(lib, policy, **kw):
    cfg, env = lc.POLICIES[policy]
    with lc._environ(env):
        return lib.Context(levels=kw.pop("levels", LEVELS), **dict(cfg, **kw))


def _submit(c, pairs, priors, s, w=W, h=H, slot=0):
    """One ugsm_submit_full_seeded of host images and host priors into NaN-filled buffers; the fields back."""
    d = Dev(c)
    try:
        put = [(d.put(L)[0], d.put(R)[0]) for L, R in pairs]
        stride = pairs[0][0].strides[0]
        dP = [c.to_device(np.ascontiguousarray(p, np.float32)) for p in priors]
        d.bufs += dP
        dO = [d.out(3 * w * h) for _ in pairs]
        c.submit_full_seeded(slot, [p[0] for p in put], [p[1] for p in put], w, h, stride, dP, s, dO)
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return [c.to_host(p, (3, h, w)) for p in dO]
    finally:
        d.free()


# ---- 1. the restriction against numpy ----------------------------------------------------------------------------------------------------

def _special_field(w, h, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 40.0, (3, h, w)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 3e38, -3e38, 1e-44, -1e-45, 1.1754942e-38, 5e-39, 0.0], np.float32)
    for p in range(3):
        at = rng.integers(0, w * h, w * h // 5)
        f[p].reshape(-1)[at] = special[rng.integers(0, len(special), len(at))]
        f[p, :3, :3] = special[:9].reshape(3, 3)                   # the first sites of every level
        f[p, 1::2, 1] = special[1 + p]
    return f


@pytest.mark.parametrize("w,h,levels", [(333, 251, 14), (231, 211, 14), (67, 49, 9)], ids=["333x251", "231x211", "67x49-nine-levels"])
def test_stage_restrict_against_numpy(lib, w, h, levels):
    f = _special_field(w, h, 9100 + w)
    lw, lh = lib.level_dims(w, h, levels)
    with lib.Context(levels=levels) as c:
        fill = np.full(3 * w * h + 64, np.nan, np.float32)      # (stays referenced while the copies read it)
        src, dst = c.to_device(f), c.to_device(fill)
        try:
            for s in range(levels):
                c.check(c.lib.ugsm_copy_to_device(c.handle, dst, fill.ctypes.data, fill.nbytes))
                c.stage_restrict(src, w, h, s, dst)
                got = c.to_host(dst, (3 * w * h + 64,))
                n3 = 3 * lw[s] * lh[s]
                assert_bit_equal(got[:n3].reshape(3, lh[s], lw[s]), sn.restrict_np(f, s, lw[s], lh[s]), f"{w}x{h}, level {s}")
                assert np.isnan(got[n3:]).all(), f"level {s}: written past the level's three planes"
            assert c.lib.ugsm_stage_restrict(c.handle, src, w, h, levels, dst) == lib.UGSM_ERR_BAD_ARG
            assert c.lib.ugsm_stage_restrict(c.handle, src, w, h, -1, dst) == lib.UGSM_ERR_BAD_ARG
            assert c.lib.ugsm_stage_restrict(c.handle, None, w, h, 0, dst) == lib.UGSM_ERR_BAD_ARG
        finally:
            c.free(src)
            c.free(dst)


# ---- 2. the call against the oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("s", STARTS)
@pytest.mark.parametrize("policy", list(lc.POLICIES))
def test_definition(lib, orc, policy, s, n):
    js = list(range(n))
    want = [_seeded(orc, j, s) for j in js]
    for j in js:
        _premise(orc, j, s, want[j])
    if n == 3:
        assert len({_prior(orc, j).tobytes() for j in js}) == 3, "premise: three different priors"
    with _context(lib, policy, batch=n) as c:
        outs = _submit(c, [lc.pairs()[j] for j in js], [_prior(orc, j) for j in js], s)
    for j in js:
        moved = np.nanmean(np.abs(want[j][:2].astype(np.float64) - _cold(orc, j)[:2]))
        print(f"{policy}, start level {s}, pair {j} of {n}: oracle seeded vs cold mean |d| = {moved:.3f} px")
        assert_bit_equal(outs[j], want[j], f"{policy}, start level {s}, pair {j} of {n}")


def test_bgr8(lib, orc):
    s, (L, R) = 5, lc.pairs()[0]
    want = _seeded(orc, 0, s)
    _premise(orc, 0, s, want)
    a, b = en.encode(L, en.BGR8), en.encode(R, en.BGR8)
    assert np.array_equal(en.to_rgb8(a, en.BGR8), L) and not np.array_equal(a, L)
    with lib.Context(levels=LEVELS) as c:
        c.set_input_format(en.BGR8)
        out = _submit(c, [(a, b)], [_prior(orc, 0)], s)[0]
        assert c.input_format == en.BGR8
    assert_bit_equal(out, want, "bgr8 images, start level 5")


def test_kernel_path_1_runs_the_pairs_one_after_the_other(lib, orc):
    """libugsm_dev.so, one kernel per reference stage: the same fields as the default path (and so the oracle's)."""
    s = 5
    pairs, priors = lc.pairs(), [_prior(orc, j) for j in range(3)]
    with lib.Context(levels=LEVELS, batch=3) as c:
        default = _submit(c, pairs, priors, s)
    with lib.Context(levels=LEVELS, kernel_path=1, dev=True, profile_events=2) as c:
        dev = _submit(c, pairs, priors, s)
        launches = sum(st["launches"] for st in c.kernel_stats() if st["name"] == "k_restrict")
    assert launches == 3, "pair by pair: one restriction per pair"
    for j in range(3):
        _premise(orc, j, s, _seeded(orc, j, s))
        assert_bit_equal(dev[j], default[j], f"kernel_path 1 against the default path, pair {j}")
        assert_bit_equal(dev[j], _seeded(orc, j, s), f"kernel_path 1 against the oracle, pair {j}")


def test_one_strip_wide_on_a_six_level_context(lib, orc):
    """59 x 45, six levels: one strip wide, the top level 10 x 7."""
    from ug_stereomatcher_amd import synth
    w, h, lv = 59, 45, 6
    L, R = synth.make_pair(w, h, synth.BASE_SEED + 7411)[:2]
    P = synth.make_pair(w, h, synth.BASE_SEED + 7412)[:2]
    prior, cold = orc.match_full(*P, lv), orc.match_full(L, R, lv)
    assert lib.level_dims(w, h, lv)[0][lv - 1] <= 10
    with lib.Context(levels=lv) as c:
        for s in (5, 2, 0):
            want = sn.seeded_oracle(orc, L, R, prior, s, lv)
            assert not np.array_equal(want.view(np.uint32), cold.view(np.uint32)), f"premise, level {s}"
            assert_bit_equal(_submit(c, [(L, R)], [prior], s, w, h)[0], want, f"59x45, six levels, start level {s}")
        d = Dev(c)
        (pl, stride), (pr, _) = d.put(L), d.put(R)
        fill = np.full(3 * w * h, np.nan, np.float32)               # (stays referenced while the copy reads it)
        o = c.to_device(fill)
        d.bufs.append(o)
        for bad in (6, -1):
            with pytest.raises(lib.UgsmError) as e:
                c.submit_full_seeded(0, [pl], [pr], w, h, stride, [o], bad, [o])
            assert e.value.status == lib.UGSM_ERR_BAD_ARG
        c.set_lr_check(1.0, lib.UGSM_LR_FULL)
        with pytest.raises(lib.UgsmError) as e:
            c.submit_full_seeded(0, [pl], [pr], w, h, stride, [o], 2, [o])
        assert e.value.status == lib.UGSM_ERR_STATE
        c.set_lr_check(0.0, 0)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert np.isnan(c.to_host(o, (3 * w * h,))).all(), "a refused call wrote nothing"
        d.free()


# ---- 3. chaining -------------------------------------------------------------------------------------------------------------------------

def test_two_calls_back_to_back_in_place(lib, orc):
    """Frame after frame on one slot, no wait in between: the second call's prior is the first's d_out, and it writes there."""
    s1, s2 = 5, 4
    f1 = _seeded(orc, 0, s1)
    f2 = _seeded(orc, 2, s2, prior=f1, key="chain")
    _premise(orc, 2, s2, f2)
    assert not np.array_equal(f2.view(np.uint32), _seeded(orc, 2, s2).view(np.uint32)), "premise: the chain's prior matters"
    with lib.Context(levels=LEVELS) as c:
        d = Dev(c)
        try:
            (l0, stride), (r0, _), (l2, _), (r2, _) = [d.put(a) for a in lc.pairs()[0] + lc.pairs()[2]]
            prior = c.to_device(_prior(orc, 0))
            d.bufs.append(prior)
            field = d.out(3 * W * H)
            c.submit_full_seeded(0, [l0], [r0], W, H, stride, [prior], s1, [field])
            c.submit_full_seeded(0, [l2], [r2], W, H, stride, [field], s2, [field])
            c.check(c.lib.ugsm_wait(c.handle, 0))
            got = c.to_host(field, (3, H, W))
        finally:
            d.free()
    assert_bit_equal(got, f2, "the second of two chained calls, in place")


# ---- 4. what runs ------------------------------------------------------------------------------------------------------------------------

def _is_level_work(name):
    return name.startswith(("k_cost", "k_smooth", "k_sqblur", "k_seed", "k_blur_decimate", "k_box", "k_warp"))


@pytest.mark.parametrize("n", [1, 3])
def test_census_at_start_level_5(lib, orc, n):
    s = 5
    lw, lh = lib.level_dims(W, H, LEVELS)
    js = list(range(n))
    with lib.Context(levels=LEVELS, slots=1, profile_events=2, batch=n) as c:
        outs = _submit(c, [lc.pairs()[j] for j in js], [_prior(orc, j) for j in js], s)
        stats = [st for st in c.kernel_stats() if st["launches"] > 0]
    for j in js:
        assert_bit_equal(outs[j], _seeded(orc, j, s), f"profiled call, pair {j}")
    above = [(st["name"], st["level"]) for st in stats if st["level"] > s and _is_level_work(st["name"])]
    assert not above, f"launches at levels above {s}: {above}"
    restrict = [st for st in stats if st["name"] == "k_restrict"]
    assert [(st["level"], st["launches"], st["pixel_launches"]) for st in restrict] == [(s, 1, float(n * lw[s] * lh[s]))], restrict
    cost = sum(st["launches"] for st in stats if st["name"].startswith("k_cost"))
    want = sum(lib.level_iterations(i) for i in range(s + 1))
    assert {st["level"] for st in stats if st["name"].startswith("k_cost")} == set(range(s + 1))
    assert cost == want, (cost, want)        # (n = 3 in lockstep: every level of this size is one launch for all the pairs)
    seeds = [st for st in stats if st["name"] == "k_seed"]
    assert all(st["level"] <= s for st in seeds), seeds      # (a seed launch is counted at the level it reads: 5 -> 4 at level 5)


# ---- 5. the blocking call ----------------------------------------------------------------------------------------------------------------

def test_match_full_seeded_from_pageable_memory(lib, orc):
    s, (L, R) = 4, lc.pairs()[1]
    want = _seeded(orc, 1, s)
    _premise(orc, 1, s, want)
    prior = np.array(_prior(orc, 1))                      # pageable, writable: the call must leave it alone
    keep = prior.copy()
    with lib.Context(levels=LEVELS) as c:
        got = c.match_full_seeded(L, R, prior, s)
        again = c.match_full_seeded(L, R, got, 0)         # ... and a second frame from the first's result
    assert_bit_equal(prior, keep, "the prior after the call")
    assert_bit_equal(got, want, "ugsm_match_full_seeded, start level 4")
    assert_bit_equal(again, _seeded(orc, 1, 0, prior=want, key="again"), "ugsm_match_full_seeded from its own result, start level 0")
    from ug_stereomatcher_amd import MatchGPULib
    m = MatchGPULib(levels=LEVELS)
    try:
        assert_bit_equal(m.matchSeeded(L, R, prior, s), want, "MatchGPULib.matchSeeded")
    finally:
        m.close()
