"""The full-mode call in two halves on the device: ugsm_stage_prolong, ugsm_submit_full_coarse, ugsm_submit_full_fine and the blocking forms.

The contract (include/ugsm.h): coarse(e) followed by fine(e) is ugsm_submit_full, bit for bit.  Either half is also pinned on its own:
d_state[k] is the field the cold call holds when level e has finished, d_full[k] its prolongation, and the fine half from ANY state of level e
is subsampleDisp of it followed by matchlevel on the levels e-1 .. 0.  tests/coarse_np.py composes exactly that of the CPU oracle's stages and a
numpy prolongation written from the definition; every comparison here is equality of float32 bit patterns (NaN where NaN).  The fine half is
also run from the NEXT pair's state, whose result the oracle shows to differ from the cold field: a fine call that ignored its state, or a test
that compared the cold field with itself, cannot pass."""
import numpy as np
import pytest

import coarse_np as cn
import encode_np as en
import launch_census as lc
import seeded_np as sn
from conftest import assert_bit_equal
from test_gpu_input_format import Dev
from test_gpu_seeded import _special_field

pytestmark = pytest.mark.gpu

W, H, LEVELS = lc.W, lc.H, lc.LEVELS          # 333 x 251: every one of the 14 levels exists
STOPS = (0, 1, 2, 5, 13)
STATES = (1, 2, 5, 13)


def _field(w, h, seed):
    """_special_field of the seeded GPU tests (NaN, +-inf, +-3e38, denormals, -0.0), cropped where a level is smaller than its 3 x 3 corner."""
    return np.ascontiguousarray(_special_field(max(w, 3), max(h, 3), seed)[:, :h, :w])


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
    p = _memo(("pyr", j), lambda: tuple(a for side in sn.pyramids(orc, *lc.pairs()[j], LEVELS) for a in side))
    return p[:LEVELS], p[LEVELS:]


def _states(orc, j):
    """Level e's field of pair j for every e, from ONE descent: what coarse_oracle(e) gives (asserted for e = 5 in test_coarse)."""
    def make():
        pl, pr = _pyr(orc, j)
        out, d = [None] * LEVELS, np.zeros_like(pl[LEVELS - 1])
        for i in range(LEVELS - 1, -1, -1):
            d, _ = orc.iterate_level(pl[i], pr[i], d, orc.iterations_for_level(i), orc.smooth_passes_for_level(i), i == LEVELS - 1)
            out[i] = d
            if i > 0:
                d = orc.seed(d, pl[i - 1].shape[2], pl[i - 1].shape[1])
        return tuple(out)
    return _memo(("states", j), make)


def _fine_from_next(orc, j, e):
    """Pair j's fine half from the state of pair j + 1: the definition, and the premise that it is not pair j's cold field."""
    f = _memo(("fine_next", j, e), lambda: cn.fine_oracle(orc, None, None, _states(orc, (j + 1) % 3)[e], e, LEVELS, _pyr(orc, j)))
    assert not np.array_equal(f.view(np.uint32), _cold(orc, j).view(np.uint32)), f"premise: pair {j} from pair {(j + 1) % 3}'s level-{e} state is its cold field"
    return f


def _dims(lib, e, w=W, h=H, levels=LEVELS):
    lw, lh = lib.level_dims(w, h, levels)
    return lw[:e + 1], lh[:e + 1]


def _context(lib, policy, **kw):
    cfg, env = lc.POLICIES[policy]
    with lc._environ(env):
        return lib.Context(levels=kw.pop("levels", LEVELS), **dict(cfg, **kw))


GUARD = 64


def _nan_buffer(c, d, nfloats):
    """A device buffer of nfloats + GUARD floats, all NaN."""
    fill = np.full(nfloats + GUARD, np.nan, np.float32)
    p = c.to_device(fill)
    d.bufs.append(p)
    return p


def _back(c, p, shape, what):
    n = int(np.prod(shape))
    got = c.to_host(p, (n + GUARD,))
    assert np.isnan(got[n:]).all(), f"{what}: written past its three planes"
    return got[:n].reshape(shape)


class _Halves:
    """The images of `pairs` on the device of context c, and the two calls into NaN-filled, guarded buffers."""

    def __init__(self, c, lib, pairs, w=W, h=H, levels=LEVELS):
        self.c, self.lib, self.w, self.h, self.levels, self.d = c, lib, w, h, levels, Dev(c)
        self.put = [(self.d.put(L)[0], self.d.put(R)[0]) for L, R in pairs]
        self.stride = pairs[0][0].strides[0]
        self.n = len(pairs)

    def coarse(self, e, full=None, wait=True, slot=0):
        """full: per pair, whether it gets a d_full entry (None: no d_full array at all).  Returns (state pointers, full pointers)."""
        lw, lh = _dims(self.lib, e, self.w, self.h, self.levels)
        dS = [_nan_buffer(self.c, self.d, 3 * lw[e] * lh[e]) for _ in range(self.n)]
        dF = None if full is None else [_nan_buffer(self.c, self.d, 3 * self.w * self.h) if f else None for f in full]
        self.c.submit_full_coarse(slot, [p[0] for p in self.put], [p[1] for p in self.put], self.w, self.h, self.stride, e, dS, dF)
        if wait:
            self.c.check(self.c.lib.ugsm_wait(self.c.handle, slot))
        return dS, dF

    def fine(self, dS, e, slot=0):
        dO = [_nan_buffer(self.c, self.d, 3 * self.w * self.h) for _ in range(self.n)]
        self.c.submit_full_fine(slot, [p[0] for p in self.put], [p[1] for p in self.put], self.w, self.h, self.stride, dS, e, dO)
        self.c.check(self.c.lib.ugsm_wait(self.c.handle, slot))
        return dO

    def state(self, p, e, what):
        lw, lh = _dims(self.lib, e, self.w, self.h, self.levels)
        return _back(self.c, p, (3, lh[e], lw[e]), what)

    def field(self, p, what):
        return _back(self.c, p, (3, self.h, self.w), what)

    def free(self):
        self.d.free()


# ---- 1. the prolongation against numpy ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,levels", [(333, 251, 14), (231, 211, 14), (67, 49, 9)], ids=["333x251", "231x211", "67x49-nine-levels"])
def test_stage_prolong_against_numpy(lib, w, h, levels):
    lw, lh = lib.level_dims(w, h, levels)
    with lib.Context(levels=levels) as c:
        fill = np.full(3 * w * h + GUARD, np.nan, np.float32)      # (stays referenced while the copies read it)
        dst = c.to_device(fill)
        try:
            for e in range(levels):
                f = _field(lw[e], lh[e], 9300 + 17 * e + w)
                src = c.to_device(f)
                c.check(c.lib.ugsm_copy_to_device(c.handle, dst, fill.ctypes.data, fill.nbytes))
                c.stage_prolong(src, w, h, e, dst)
                got = c.to_host(dst, (3 * w * h + GUARD,))
                c.free(src)
                assert_bit_equal(got[:3 * w * h].reshape(3, h, w), cn.prolong_np(f, (lw[:e + 1], lh[:e + 1])), f"{w}x{h}, level {e}")
                assert np.isnan(got[3 * w * h:]).all(), f"level {e}: written past the three planes"
            assert c.lib.ugsm_stage_prolong(c.handle, dst, w, h, levels, dst) == lib.UGSM_ERR_BAD_ARG
            assert c.lib.ugsm_stage_prolong(c.handle, dst, w, h, -1, dst) == lib.UGSM_ERR_BAD_ARG
            assert c.lib.ugsm_stage_prolong(c.handle, None, w, h, 0, dst) == lib.UGSM_ERR_BAD_ARG
            assert c.lib.ugsm_stage_prolong(c.handle, dst, w, h, 0, None) == lib.UGSM_ERR_BAD_ARG
        finally:
            c.free(dst)


@pytest.mark.parametrize("w,shift", [(332, 0), (332, 2), (334, 0), (334, 1)], ids=["16-byte-rows", "8-byte-base", "8-byte-rows", "4-byte-base"])
def test_stage_prolong_at_every_store_width(lib, w, shift):
    """Rows of a multiple of four floats, of two, and output bases that spoil either: the same field through each of the kernel's store forms."""
    h, levels, e = 37, 9, 3
    lw, lh = lib.level_dims(w, h, levels)
    f = _field(lw[e], lh[e], 77 + w)
    with lib.Context(levels=levels) as c:
        fill = np.full(3 * w * h + GUARD, np.nan, np.float32)
        src, dst = c.to_device(f), c.to_device(fill)
        try:
            c.stage_prolong(src, w, h, e, dst + 4 * shift)
            got = c.to_host(dst, (3 * w * h + GUARD,))
        finally:
            c.free(src)
            c.free(dst)
    assert np.isnan(got[:shift]).all() and np.isnan(got[shift + 3 * w * h:]).all(), "written outside the three planes"
    assert_bit_equal(got[shift:shift + 3 * w * h].reshape(3, h, w), cn.prolong_np(f, (lw[:e + 1], lh[:e + 1])), f"{w} wide, base + {shift} floats")


def test_stage_prolong_three_workgroups_across(lib):
    """2052 x 1367: three workgroups of 1024 columns across, the last of them all but four columns outside the row."""
    w, h, levels = 2052, 1367, 14
    lw, lh = lib.level_dims(w, h, levels)
    with lib.Context(levels=levels) as c:
        fill = np.full(3 * w * h + GUARD, np.nan, np.float32)
        dst = c.to_device(fill)
        try:
            for e in (1, 4):
                f = _field(lw[e], lh[e], 555 + e)
                src = c.to_device(f)
                c.check(c.lib.ugsm_copy_to_device(c.handle, dst, fill.ctypes.data, fill.nbytes))
                c.stage_prolong(src, w, h, e, dst)
                got = c.to_host(dst, (3 * w * h + GUARD,))
                c.free(src)
                assert_bit_equal(got[:3 * w * h].reshape(3, h, w), cn.prolong_np(f, (lw[:e + 1], lh[:e + 1])), f"{w}x{h}, level {e}")
                assert np.isnan(got[3 * w * h:]).all(), f"level {e}: written past the three planes"
        finally:
            c.free(dst)


# ---- 2. the coarse half ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("e", STOPS)
@pytest.mark.parametrize("policy", list(lc.POLICIES))
def test_coarse(lib, orc, policy, e, n):
    js = list(range(n))
    want = [_states(orc, j)[e] for j in js]
    if e == 5:
        assert_bit_equal(want[0], cn.coarse_oracle(orc, None, None, e, LEVELS, _pyr(orc, 0)), "the shared descent against coarse_oracle")
    if e == 0:
        for j in js:
            assert_bit_equal(want[j], _cold(orc, j), f"oracle: level 0's field of pair {j} is orc.match_full")
    full = [True] if n == 1 else [True, False, True]
    with _context(lib, policy, batch=n) as c:
        hv = _Halves(c, lib, [lc.pairs()[j] for j in js])
        try:
            dS, dF = hv.coarse(e, full)
            states = [hv.state(dS[j], e, f"d_state[{j}]") for j in js]
            fulls = [hv.field(dF[j], f"d_full[{j}]") if full[j] else None for j in js]
        finally:
            hv.free()
    for j in js:
        assert_bit_equal(states[j], want[j], f"{policy}, stop level {e}, pair {j} of {n}: d_state")
        if full[j]:
            assert_bit_equal(fulls[j], cn.prolong_np(want[j], _dims(lib, e)), f"{policy}, stop level {e}, pair {j} of {n}: d_full")


def test_coarse_without_a_full_array(lib, orc):
    with lib.Context(levels=LEVELS) as c:
        hv = _Halves(c, lib, lc.pairs()[:2])
        try:
            dS, _ = hv.coarse(5, None)
            for j in range(2):
                assert_bit_equal(hv.state(dS[j], 5, f"d_state[{j}]"), _states(orc, j)[5], f"no d_full, pair {j}")
        finally:
            hv.free()


# ---- 3. the fine half --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("e", STATES)
@pytest.mark.parametrize("policy", list(lc.POLICIES))
def test_fine(lib, orc, policy, e, n):
    js = list(range(n))
    other = [_fine_from_next(orc, j, e) for j in js]
    with _context(lib, policy, batch=n) as c:
        hv = _Halves(c, lib, [lc.pairs()[j] for j in js])
        try:
            dS, _ = hv.coarse(e, None, wait=False)               # the two halves on one slot, no wait in between
            own = [hv.field(p, "d_out") for p in hv.fine(dS, e)]
            dN =[c.to_device(np.ascontiguousarray(_states(orc, (j + 1) % 3)[e])) for j in js]
            hv.d.bufs += dN
            nxt = [hv.field(p, "d_out") for p in hv.fine(dN, e)]
        finally:
            hv.free()
    for j in js:
        assert_bit_equal(own[j], _cold(orc, j), f"{policy}, state level {e}, pair {j} of {n}: fine(coarse) against orc.match_full")
        assert_bit_equal(nxt[j], other[j], f"{policy}, state level {e}, pair {j} of {n}: from the next pair's state")


# ---- 4. another input format, the other kernel path, a narrow size -----------------------------------------------------------------------

def test_bgr8(lib, orc):
    e, (L, R) = 5, lc.pairs()[0]
    a, b = en.encode(L, en.BGR8), en.encode(R, en.BGR8)
    assert np.array_equal(en.to_rgb8(a, en.BGR8), L) and not np.array_equal(a, L)
    with lib.Context(levels=LEVELS) as c:
        c.set_input_format(en.BGR8)
        hv = _Halves(c, lib, [(a, b)])
        try:
            dS, dF = hv.coarse(e, [True], wait=False)
            out = hv.field(hv.fine(dS, e)[0], "d_out")
            state, full = hv.state(dS[0], e, "d_state"), hv.field(dF[0], "d_full")
            assert c.input_format == en.BGR8
        finally:
            hv.free()
    assert_bit_equal(state, _states(orc, 0)[e], "bgr8 images: d_state")
    assert_bit_equal(full, cn.prolong_np(_states(orc, 0)[e], _dims(lib, e)), "bgr8 images: d_full")
    assert_bit_equal(out, _cold(orc, 0), "bgr8 images: fine(coarse)")


def test_kernel_path_1_runs_the_pairs_one_after_the_other(lib, orc):
    """libugsm_dev.so, one kernel per reference stage: the same fields as the default path (and so the oracle's)."""
    e = 5

    def both(c):
        hv = _Halves(c, lib, lc.pairs())
        try:
            dS, dF = hv.coarse(e, [True, False, True], wait=False)
            outs = [hv.field(p, "d_out") for p in hv.fine(dS, e)]
            return [hv.state(p, e, "d_state") for p in dS], [hv.field(p, "d_full") if p else None for p in dF], outs
        finally:
            hv.free()
    with lib.Context(levels=LEVELS, batch=3) as c:
        default = both(c)
    with lib.Context(levels=LEVELS, kernel_path=1, dev=True, profile_events=2) as c:
        dev = both(c)
        launches = sum(st["launches"] for st in c.kernel_stats() if st["name"] == "k_prolong")
    assert launches == 2, "pair by pair: one prolongation per pair that asked"
    for j in range(3):
        assert_bit_equal(dev[0][j], default[0][j], f"kernel_path 1 against the default path, pair {j}: d_state")
        assert_bit_equal(dev[0][j], _states(orc, j)[e], f"kernel_path 1 against the oracle, pair {j}: d_state")
        if j != 1:
            assert_bit_equal(dev[1][j], default[1][j], f"kernel_path 1 against the default path, pair {j}: d_full")
        assert_bit_equal(dev[2][j], default[2][j], f"kernel_path 1 against the default path, pair {j}: d_out")
        assert_bit_equal(dev[2][j], _cold(orc, j), f"kernel_path 1 against the oracle, pair {j}: d_out")


def test_one_strip_wide_on_a_six_level_context(lib, orc):
    """59 x 45, six levels: one strip wide, the top level 10 x 7."""
    from ug_stereomatcher_amd import synth
    w, h, lv = 59, 45, 6
    L, R = synth.make_pair(w, h, synth.BASE_SEED + 7411)[:2]
    P = synth.make_pair(w, h, synth.BASE_SEED + 7412)[:2]
    cold = orc.match_full(L, R, lv)
    pyr, pyrP = sn.pyramids(orc, L, R, lv), sn.pyramids(orc, *P, lv)
    assert lib.level_dims(w, h, lv)[0][lv - 1] <= 10
    with lib.Context(levels=lv) as c:
        hv = _Halves(c, lib, [(L, R)], w, h, lv)
        try:
            for e in (5, 2):
                want = cn.coarse_oracle(orc, L, R, e, lv, pyr)
                dS, dF = hv.coarse(e, [True])
                assert_bit_equal(hv.state(dS[0], e, "d_state"), want, f"59x45, six levels, stop level {e}: d_state")
                assert_bit_equal(hv.field(dF[0], "d_full"), cn.prolong_np(want, _dims(lib, e, w, h, lv)), f"59x45, six levels, stop level {e}: d_full")
            for e in (5, 1):
                dS, _ = hv.coarse(e, None, wait=False)
                assert_bit_equal(hv.field(hv.fine(dS, e)[0], "d_out"), cold, f"59x45, six levels, state level {e}: fine(coarse)")
                stateP = cn.coarse_oracle(orc, *P, e, lv, pyrP)
                want = cn.fine_oracle(orc, L, R, stateP, e, lv, pyr)
                assert not np.array_equal(want.view(np.uint32), cold.view(np.uint32)), f"premise, level {e}"
                dP = c.to_device(stateP)
                hv.d.bufs.append(dP)
                assert_bit_equal(hv.field(hv.fine([dP], e)[0], "d_out"), want, f"59x45, six levels, state level {e}: from another pair's state")
            # refused calls write nothing
            (pl, pr) = hv.put[0]
            o = _nan_buffer(c, hv.d, 3 * w * h)
            st = _nan_buffer(c, hv.d, 3 * w * h)
            for bad in (6, -1):
                with pytest.raises(lib.UgsmError) as err:
                    c.submit_full_coarse(0, [pl], [pr], w, h, hv.stride, bad, [st], [o])
                assert err.value.status == lib.UGSM_ERR_BAD_ARG
            for bad in (6, 0, -1):
                with pytest.raises(lib.UgsmError) as err:
                    c.submit_full_fine(0, [pl], [pr], w, h, hv.stride, [st], bad, [o])
                assert err.value.status == lib.UGSM_ERR_BAD_ARG
            with pytest.raises(lib.UgsmError) as err:
                c.submit_full_coarse(0, [pl], [pr], w, h, hv.stride, 0, [st], [st + 4])    # d_full over the call's own state
            assert err.value.status == lib.UGSM_ERR_BAD_ARG
            c.set_lr_check(1.0, lib.UGSM_LR_FULL)
            with pytest.raises(lib.UgsmError) as err:
                c.submit_full_coarse(0, [pl], [pr], w, h, hv.stride, 2, [st], [o])
            assert err.value.status == lib.UGSM_ERR_STATE
            with pytest.raises(lib.UgsmError) as err:
                c.submit_full_fine(0, [pl], [pr], w, h, hv.stride, [st], 2, [o])
            assert err.value.status == lib.UGSM_ERR_STATE
            c.set_lr_check(0.0, 0)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            for p in (o, st):
                assert np.isnan(c.to_host(p, (3 * w * h + GUARD,))).all(), "a refused call wrote something"
        finally:
            hv.free()


# ---- 5. what runs ------------------------------------------------------------------------------------------------------------------------

def _is_level_work(name):
    return name.startswith(("k_cost", "k_smooth", "k_sqblur", "k_seed", "k_box", "k_warp"))


@pytest.mark.parametrize("n", [1, 3])
def test_census_at_level_5(lib, orc, n):
    e = 5
    js = list(range(n))
    with lib.Context(levels=LEVELS, slots=1, profile_events=2, batch=n) as c:
        hv = _Halves(c, lib, [lc.pairs()[j] for j in js])
        try:
            dS, dF = hv.coarse(e, [True] * n)
            coarse = [st for st in c.kernel_stats() if st["launches"] > 0]
            c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
            outs = [hv.field(p, "d_out") for p in hv.fine(dS, e)]
            fine = [st for st in c.kernel_stats() if st["launches"] > 0]
            fulls = [hv.field(p, "d_full") for p in dF]
        finally:
            hv.free()
    for j in js:
        assert_bit_equal(outs[j], _cold(orc, j), f"profiled halves, pair {j}")
        assert_bit_equal(fulls[j], cn.prolong_np(_states(orc, j)[e], _dims(lib, e)), f"profiled coarse call, pair {j}: d_full")
    # the coarse half: nothing of a level below 5, one prolongation, the K-cost launches of the levels 5 .. 13
    below = [(st["name"], st["level"]) for st in coarse if st["level"] < e and _is_level_work(st["name"])]
    assert not below, f"coarse: level work at levels below {e}: {below}"
    prolong = [(st["level"], st["launches"], st["pixel_launches"]) for st in coarse if st["name"] == "k_prolong"]
    assert prolong == [(e, 1, float(n * W * H))], prolong
    cost = [st for st in coarse if st["name"].startswith("k_cost")]
    assert {st["level"] for st in cost} == set(range(e, LEVELS))
    assert sum(st["launches"] for st in cost) == sum(lib.level_iterations(i) for i in range(e, LEVELS))
    # the fine half: no K-cost or K-smooth at the levels 5 and above, no prolongation, the K-cost launches of the levels 0 .. 4
    above = [(st["name"], st["level"]) for st in fine if st["level"] >= e and st["level"] < LEVELS and st["name"].startswith(("k_cost", "k_smooth", "k_sqblur", "k_box"))]
    assert not above, f"fine: K-cost or K-smooth at levels {e} and above: {above}"
    assert not [st for st in fine if st["name"] == "k_prolong"]
    cost = [st for st in fine if st["name"].startswith("k_cost")]
    assert {st["level"] for st in cost} == set(range(e))
    assert sum(st["launches"] for st in cost) == sum(lib.level_iterations(i) for i in range(e))
    seeds = [st for st in fine if st["name"] == "k_seed"]
    assert all(st["level"] <= e for st in seeds), seeds      # (a seed launch is counted at the level it reads: 5 -> 4 at level 5)


# ---- 6. the blocking calls ---------------------------------------------------------------------------------------------------------------

def test_match_full_coarse_and_fine_from_pageable_memory(lib, orc):
    e, (L, R) = 5, lc.pairs()[1]
    with lib.Context(levels=LEVELS) as c:
        state, full = c.match_full_coarse(L, R, e, want_full=True)
        alone = c.match_full_coarse(L, R, 2)
        keep = state.copy()
        got = c.match_full_fine(L, R, state, e)
        nxt = c.match_full_fine(L, R, np.array(_states(orc, 2)[e]), e)
    assert_bit_equal(state, _states(orc, 1)[e], "ugsm_match_full_coarse, stop level 5: the state")
    assert_bit_equal(full, cn.prolong_np(_states(orc, 1)[e], _dims(lib, e)), "ugsm_match_full_coarse, stop level 5: the prolongation")
    assert_bit_equal(alone, _states(orc, 1)[2], "ugsm_match_full_coarse, stop level 2, no full planes")
    assert_bit_equal(state, keep, "the state after the fine call")
    assert_bit_equal(got, _cold(orc, 1), "ugsm_match_full_fine from the coarse call's state")
    assert_bit_equal(nxt, _fine_from_next(orc, 1, e), "ugsm_match_full_fine from the next pair's state")
    from ug_stereomatcher_amd import MatchGPULib
    m = MatchGPULib(levels=LEVELS)
    try:
        s2, f2 = m.matchCoarse(L, R, e, want_full=True)
        assert_bit_equal(s2, state, "MatchGPULib.matchCoarse: the state")
        assert_bit_equal(f2, full, "MatchGPULib.matchCoarse: the prolongation")
        assert_bit_equal(m.matchCoarse(L, R, e), state, "MatchGPULib.matchCoarse without want_full")
        assert_bit_equal(m.matchFine(L, R, s2, e), _cold(orc, 1), "MatchGPULib.matchFine")
    finally:
        m.close()
