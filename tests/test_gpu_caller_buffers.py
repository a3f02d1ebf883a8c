"""Caller-owned float buffers at 4-byte bases between guard bands (include/ugsm.h: "float buffers need 4-byte alignment and nothing more").

Several kernels choose a 16-byte or 8-byte access form from a level's WIDTH alone; a caller's buffer at base + 4, + 8 or + 12 bytes is where
such a form would meet an address the compiler was told is aligned.  Where that happens today (ugsm_full.cpp, ugsm_levels.cpp):
  * K-smooth's quad store (k_smooth_fused, st_quad<true> when W % 4 == 0): level 0's last launch of a full-mode call writes d_out / d_back /
    d_state of level 0 itself (enqueue_descent's direct_out).  The template instances are compiled one by one, so the full-mode calls run once
    per tile class -- the 112-column tile at its fixed height of 36 rows and at a variable one, 64 x 32, 32 x 16 -- under the switches of
    tests/test_gpu_smooth_io.py, the class asserted from lib.plan_level;
  * the kernels that read a caller's field in place (K-cost on d_L3 / d_R3, the restriction, the prolongation, the warm start, the warp,
    the residual, the triangulation, the clouds, the reconstruction) and those that store one float at a time.
Where it does NOT happen: the pyramid kernels' column phase always writes the slot's own pyramids (ugsm_stage_pyramid and the d_pyrL / d_pyrR
stacks are copies of them), and ugsm_stage_smooth and ugsm_stage_iterate (d_d3) copy the caller's field into the slot's buffers and back -- those
cases pin the contract of the entry point (the right floats, nothing outside them), not a kernel's access form.
Every entry point that reads or writes a caller's float buffer runs here with all of its float buffers
  * at shift 0 (the 16-byte base every other test uses), all at shift 1 (a 4-byte base), and mixed (outputs at 3, inputs at 2, then on
    through the residues), in batched calls each pair in an allocation of its own;
  * between two guard bands of GUARD poisoned floats (tests/guarded.py): a store in front of a buffer or behind it fails the test with the
    guard message, and so does a call that writes one of its inputs.
The expected values are those of the entry point's own test -- the CPU oracle or the numpy restatements -- never a second run of the
library at an aligned base; every comparison is equality of float32 bit patterns (NaN where NaN).

Sizes: the class that matters is width = 0 (mod 4), where the aligned forms are chosen: 448 x 150, 112 x 36 (exactly one 112-column tile) and
100 x 30 (smaller than a tile); 450 x 152 for the 8-byte forms; 451 x 149 as the odd control.  The residues are asserted, so that a later
change of sizes cannot turn the file into the easy case, and so is the kernel each case means to reach (lib.plan_level)."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import coarse_np as co
import fovea_seeded_np as fs
import launch_census as lc
import reconstruct_multi_np as rm
import seeded_np as sn
import stack_cloud_np as sc
import warp_np as wn
from conftest import assert_bit_equal
from guarded import POISON, Guards
from test_gpu_cloud import P1, P2A
from test_gpu_smooth_io import CLASS_ENV, expected, field

pytestmark = pytest.mark.gpu

LEVELS = 6
QUAD, PAIR_W, ODD = (448, 150), (450, 152), (451, 149)
ONE_TILE, SUB_TILE = (112, 36), (100, 30)
SIZES = [QUAD, PAIR_W, ONE_TILE, SUB_TILE, ODD]
RESIDUE = {QUAD: 0, PAIR_W: 2, ONE_TILE: 0, SUB_TILE: 0, ODD: 3}
# (W, H, levels, F) -> (fovW, fovH): one window of a multiple of four columns, one of 4 k + 2, both under 200 columns
FOVEA = {"fovW-112": ((320, 240, 8, 4), (112, 84)), "fovW-142": ((404, 300, 8, 4), (142, 105))}
OFFS2 = [(-60, 35), (40, -25)]                   # two windows, both off-centre
TAU = 1.0

# K-cost / K-smooth of level 0 by the development switches of test_gpu_march.py, test_gpu_march4.py, test_gpu_small.py and test_gpu_smooth_io.py:
# name -> (ugsm_config fields, overrides read at ugsm_create under UGSM_DEV=1, the (cost_kernel, smooth_kernel) that must be planned)
MARCH, SMALL, MARCH4, FUSED = 1, 2, 4, 0
POLICIES = {
    "default": ({}, {}, None),
    "march": (dict(march_min_pixels=1), {}, dict(cost_kernel=MARCH, smooth_kernel=FUSED)),
    "march4": (dict(small_max_pixels=-1), {"UGSM_MARCH4": "1,2000000000"}, dict(cost_kernel=MARCH4, smooth_kernel=FUSED)),
    "small": ({}, {"UGSM_SMALL_MASK": "1"}, dict(cost_kernel=SMALL, smooth_kernel=FUSED)),          # k_cost_small hands level 0 to k_smooth_fused
    # k_smooth_fused's tile class, as CLASS_ENV of test_gpu_smooth_io.py forces it on every level; the 112-column tile at 36 rows is the
    # fixed-height instance (FIXH), at 20 rows the variable-height one
    "tile-112x36": ({}, dict(CLASS_ENV["112"], UGSM_SMOOTH_ROWS="36"), dict(smooth_kernel=FUSED, smooth_tile_rows=36)),
    "tile-112x20": ({}, dict(CLASS_ENV["112"], UGSM_SMOOTH_ROWS="20"), dict(smooth_kernel=FUSED, smooth_tile_rows=20)),
    "tile-64x32": ({}, CLASS_ENV["64x32"], dict(smooth_kernel=FUSED, smooth_tile_rows=0)),
    "tile-32x16": ({}, CLASS_ENV["32x16"], dict(smooth_kernel=FUSED, smooth_tile_rows=0)),
}
TILE_POLICIES = [p for p in POLICIES if p.startswith("tile-")]
SCHEMES = ("all-0", "all-1", "mixed")


class Shifts:
    """The shift of a call's next output / input buffer under a scheme."""

    def __init__(self, scheme):
        self.scheme, self.n_out, self.n_in = scheme, 0, 0

    def out(self):
        self.n_out += 1
        return {"all-0": 0, "all-1": 1}.get(self.scheme, (3, 1, 2, 0)[(self.n_out - 1) % 4])

    def inp(self):
        self.n_in += 1
        return {"all-0": 0, "all-1": 1}.get(self.scheme, (2, 3, 1, 0)[(self.n_in - 1) % 4])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


# ---- inputs and the oracle's answers, computed once and shared, never written to ---------------------------------------------------------

_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        v = make()
        for a in (v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _MEMO[key] = v
    return _MEMO[key]


def _pair(W, H, j=0):
    def make():
        from ug_stereomatcher_amd import synth
        L, R = synth.make_pair(W, H, synth.BASE_SEED + 8800 + 13 * j)[:2]
        return np.ascontiguousarray(L), np.ascontiguousarray(R)
    return _memo(("pair", W, H, j), make)


def _cold(orc, W, H, j, levels=LEVELS):
    return _memo(("cold", W, H, j, levels), lambda: orc.match_full(*_pair(W, H, j), levels))


def _back(orc, W, H, j):
    L, R = _pair(W, H, j)
    return _memo(("back", W, H, j), lambda: orc.match_full(R, L, LEVELS))


def _pyr(orc, W, H, j, levels=LEVELS):
    p = _memo(("pyr", W, H, j, levels), lambda: tuple(a for side in sn.pyramids(orc, *_pair(W, H, j), levels) for a in side))
    return p[:levels], p[levels:]


def _fov_cold(orc, cfg, j, off, want_pyr=False):
    W, H, lv, F = cfg
    return _memo(("fov", cfg, j, tuple(off)), lambda: orc.match_foveated(*_pair(W, H, j), lv, F, off[0], off[1], want_pyr=True))[:3 if want_pyr else 1]


def _fov_back(orc, cfg, j, off):
    W, H, lv, F = cfg
    L, R = _pair(W, H, j)
    return _memo(("fov-back", cfg, j, tuple(off)), lambda: orc.match_foveated(R, L, lv, F, off[0], off[1])[0])


def _finite_field(W, H, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(0, 5, (H, W)), rng.normal(0, 4, (H, W)), 0.05 + 0.95 * rng.random((H, W))]).astype(np.float32)


def _context(lib, policy="default", levels=LEVELS, size=None, launch_pairs=None, **kw):
    """A context under `policy`; with `size`, the assertion that level 0 of a call on it -- one launch of launch_pairs pairs (default: the
    context's batch) -- is planned for the kernels the policy names."""
    cfg, env, planned = POLICIES[policy]
    with lc._environ(env):
        if size is not None and planned is not None:
            pairs = launch_pairs or kw.get("batch", 0)
            plan = lib.plan_level(size[0], size[1], alone=True, **dict(cfg, batch=pairs))
            assert {k: plan[k] for k in planned} == planned, f"{policy} at {size}, {pairs} pairs per launch: {plan}"
            if policy in ("tile-64x32", "tile-32x16"):
                # the plan names no class below the 112-column tile: the launcher's rule (launch_smooth_fused, smooth_class_for) restated --
                # 64 x 32 from UGSM_SMOOTH_MID_MIN pixels per launch, a launch of several pairs also at least 48 x 24; else 32 x 16
                px = size[0] * size[1] * max(pairs, 1)
                mid = px >= int(env["UGSM_SMOOTH_MID_MIN"]) and (pairs <= 1 or (size[0] >= 48 and size[1] >= 24))
                assert mid == (policy == "tile-64x32"), f"{policy} at {size}, {pairs} pairs per launch"
        return lib.Context(levels=levels, **dict(cfg, **kw))


def _wait(c, slot=0):
    c.check(c.lib.ugsm_wait(c.handle, slot))


def _residue(size):
    assert size[0] % 4 == RESIDUE[size], f"{size}: the width's residue mod 4 is what this size is here for"


def _fovea(lib, name):
    cfg, fov = FOVEA[name]
    assert lib.fovea_dims(*cfg) == fov and fov[0] < 200 and fov[0] % 4 == (0 if name == "fovW-112" else 2), (name, lib.fovea_dims(*cfg))
    return cfg, fov


# ==== full mode ===========================================================================================================================

# every size under the context's own policy; level 0 forced to each K-cost kernel -- the kernel that hands it to the last K-smooth launch -- at
# the two multi-tile sizes; every tile class of that last launch at the widths of a multiple of four and at 450
FULL_CASES = ([(s, "default") for s in SIZES] + [(s, p) for s in (QUAD, PAIR_W) for p in ("march", "march4", "small")]
              + [(s, p) for p in TILE_POLICIES for s in (QUAD, ONE_TILE, SUB_TILE, PAIR_W)])
FULL_IDS = [f"{s[0]}x{s[1]}-{p}" for s, p in FULL_CASES]


@pytest.mark.parametrize("size,policy", FULL_CASES, ids=FULL_IDS)
def test_submit_full(lib, orc, size, policy):
    W, H = size
    _residue(size)
    L, R = _pair(W, H)
    want = _cold(orc, W, H, 0)
    with _context(lib, policy, size=size) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR, dO = g.image(L), g.image(R), g.buf(3 * W * H, sh.out())
                c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, dO))
                _wait(c)
                assert_bit_equal(g.check(dO, (3, H, W), f"{policy} {scheme} d_out"), want, f"ugsm_submit_full {W}x{H} {policy} {scheme}")
            finally:
                g.done()


BATCH_CASES = [(s, p) for s in (QUAD, PAIR_W) for p in ("default", "small")] + [(s, p) for p in TILE_POLICIES for s in (QUAD, ONE_TILE, SUB_TILE, PAIR_W)]


@pytest.mark.parametrize("size,policy", BATCH_CASES, ids=[f"{s[0]}x{s[1]}-{p}" for s, p in BATCH_CASES])
def test_submit_full_batch_of_three_in_one_launch(lib, orc, monkeypatch, size, policy):
    W, H = size
    _residue(size)
    monkeypatch.setenv("UGSM_BATCH_MAX_PIXELS", "20000000")
    pairs = [_pair(W, H, j) for j in range(3)]
    cfg, env, _ = POLICIES[policy]
    with lc._environ(env):
        plan = lib.plan_level(W, H, alone=True, batch=3, **cfg)
    assert plan["pairs_per_launch"] == 3 and plan["smooth_kernel"] == FUSED, f"level 0 is one launch of k_smooth_fused for three pairs: {plan}"
    with _context(lib, policy, size=size if policy in TILE_POLICIES else None, batch=3) as c:      # (three pairs per launch: K-cost is march4's whatever the policy)
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = [g.image(a) for a, _ in pairs], [g.image(b) for _, b in pairs]
                dO = [g.buf(3 * W * H, sh.out()) for _ in pairs]
                c.submit_full_batch(0, dL, dR, W, H, 3 * W, dO)
                _wait(c)
                for j in range(3):
                    assert_bit_equal(g.check(dO[j], (3, H, W), f"{scheme} d_out[{j}]"), _cold(orc, W, H, j), f"batch {W}x{H} {policy} {scheme}, pair {j}")
            finally:
                g.done()


@pytest.mark.parametrize("size,policy", FULL_CASES, ids=FULL_IDS)
def test_submit_full_checked(lib, orc, size, policy):
    W, H = size
    _residue(size)
    n = 1 if policy in ("march", "march4", "small") else 2          # (both directions in lockstep: 2 n pairs per launch)
    want = []
    for j in range(n):
        F_, B_ = _cold(orc, W, H, j), _back(orc, W, H, j)
        (cF, nF), (cB, nB) = orc.lr_check(F_, B_, TAU), orc.lr_check(B_, F_, TAU)
        assert 0 < nF < W * H and 0 < nB < W * H, "premise: the check fires and spares in both directions"
        want.append((np.stack([F_[0], F_[1], cF[2]]), np.stack([B_[0], B_[1], cB[2]]), (nF, nB)))
    with _context(lib, policy, size=size, launch_pairs=2 * n, batch=n) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = [g.image(_pair(W, H, j)[0]) for j in range(n)], [g.image(_pair(W, H, j)[1]) for j in range(n)]
                dO = [g.buf(3 * W * H, sh.out()) for _ in range(n)]
                dB = [g.buf(3 * W * H, sh.out()) for _ in range(n)]
                c.submit_full_checked(0, dL, dR, W, H, 3 * W, dO, dB, TAU)
                _wait(c)
                for j in range(n):
                    assert_bit_equal(g.check(dO[j], (3, H, W), f"{scheme} d_out[{j}]"), want[j][0], f"checked {W}x{H} {policy} {scheme}, pair {j}, forward")
                    assert_bit_equal(g.check(dB[j], (3, H, W), f"{scheme} d_back[{j}]"), want[j][1], f"checked {W}x{H} {policy} {scheme}, pair {j}, backward")
                    assert c.last_lr_marked_pair(0, j) == want[j][2]
            finally:
                g.done()


@pytest.mark.parametrize("size,policy", FULL_CASES, ids=FULL_IDS)
def test_submit_full_seeded(lib, orc, size, policy):
    W, H = size
    _residue(size)
    n, s = 2, 3
    priors = [_cold(orc, W, H, (j + 1) % 3) for j in range(n)]
    want = [_memo(("seeded", W, H, j, s), lambda: sn.seeded_oracle(orc, None, None, priors[j], s, LEVELS, _pyr(orc, W, H, j))) for j in range(n)]
    for j in range(n):
        assert not np.array_equal(want[j].view(np.uint32), _cold(orc, W, H, j).view(np.uint32)), "premise: the seeded field is not the cold one"
    with _context(lib, policy, size=size, batch=n) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = [g.image(_pair(W, H, j)[0]) for j in range(n)], [g.image(_pair(W, H, j)[1]) for j in range(n)]
                dP = [g.inp(p, sh.inp()) for p in priors]
                dO = [g.buf(3 * W * H, sh.out()) for _ in range(n)]
                c.submit_full_seeded(0, dL, dR, W, H, 3 * W, dP, s, dO)
                _wait(c)
                for j in range(n):
                    assert_bit_equal(g.check(dO[j], (3, H, W), f"{scheme} d_out[{j}]"), want[j], f"seeded {W}x{H} {policy} {scheme}, pair {j}")
            finally:
                g.done(f"seeded {scheme}")


def _state(orc, W, H, j, e):
    return _memo(("state", W, H, j, e), lambda: co.coarse_oracle(orc, None, None, e, LEVELS, _pyr(orc, W, H, j)))


COARSE_CASES = [(s, 2, "default") for s in SIZES] + [(s, 0, p) for s, p in FULL_CASES if s in (QUAD, PAIR_W) or p in TILE_POLICIES]    # e = 0: the whole call


@pytest.mark.parametrize("size,e,policy", COARSE_CASES, ids=[f"{s[0]}x{s[1]}-e{e}-{p}" for s, e, p in COARSE_CASES])
def test_submit_full_coarse(lib, orc, size, e, policy):
    W, H = size
    _residue(size)
    n = 2
    lw, lh = lib.level_dims(W, H, LEVELS)
    if e == 2 and size in (QUAD, PAIR_W):
        assert lw[2] % 4 == (3 if size == QUAD else 0), lw          # the state's own width: odd, and a multiple of four
    states = [_state(orc, W, H, j, e) for j in range(n)]
    fulls = [co.prolong_np(st, (lw[:e + 1], lh[:e + 1])) for st in states]
    with _context(lib, policy, size=size, batch=n) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = [g.image(_pair(W, H, j)[0]) for j in range(n)], [g.image(_pair(W, H, j)[1]) for j in range(n)]
                dS = [g.buf(3 * lw[e] * lh[e], sh.out()) for _ in range(n)]
                dF = [g.buf(3 * W * H, sh.out()) for _ in range(n)]
                c.submit_full_coarse(0, dL, dR, W, H, 3 * W, e, dS, dF)
                _wait(c)
                for j in range(n):
                    assert_bit_equal(g.check(dS[j], (3, lh[e], lw[e]), f"{scheme} d_state[{j}]"), states[j], f"coarse {W}x{H} e={e} {policy} {scheme}, state {j}")
                    assert_bit_equal(g.check(dF[j], (3, H, W), f"{scheme} d_full[{j}]"), fulls[j], f"coarse {W}x{H} e={e} {policy} {scheme}, prolongation {j}")
            finally:
                g.done()


@pytest.mark.parametrize("size,policy", FULL_CASES, ids=FULL_IDS)
def test_submit_full_fine(lib, orc, size, policy):
    W, H = size
    _residue(size)
    n, e = 2, 2
    lw, lh = lib.level_dims(W, H, LEVELS)
    states = [_state(orc, W, H, (j + 1) % 3, e) for j in range(n)]          # another pair's state: a fine half that ignored it cannot pass
    want = [_memo(("fine", W, H, j, e), lambda: co.fine_oracle(orc, None, None, states[j], e, LEVELS, _pyr(orc, W, H, j))) for j in range(n)]
    for j in range(n):
        assert not np.array_equal(want[j].view(np.uint32), _cold(orc, W, H, j).view(np.uint32)), "premise: not the cold field"
    with _context(lib, policy, size=size, batch=n) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = [g.image(_pair(W, H, j)[0]) for j in range(n)], [g.image(_pair(W, H, j)[1]) for j in range(n)]
                dS = [g.inp(st, sh.inp()) for st in states]
                dO = [g.buf(3 * W * H, sh.out()) for _ in range(n)]
                c.submit_full_fine(0, dL, dR, W, H, 3 * W, dS, e, dO)
                _wait(c)
                for j in range(n):
                    assert_bit_equal(g.check(dO[j], (3, H, W), f"{scheme} d_out[{j}]"), want[j], f"fine {W}x{H} {policy} {scheme}, pair {j}")
            finally:
                g.done(f"fine {scheme}")


# ==== foveated ============================================================================================================================

@pytest.mark.parametrize("name", list(FOVEA))
def test_submit_foveated_with_both_pyramid_stacks(lib, orc, name):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    L, R = _pair(W, H)
    off = OFFS2[0]
    stack, pl, pr = _fov_cold(orc, cfg, 0, off, want_pyr=True)
    nf = 3 * F * fh * fw
    with lib.Context(levels=lv, fovea_levels=F) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = g.image(L), g.image(R)
                dS, dPL, dPR = (g.buf(nf, sh.out()) for _ in range(3))
                c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dL, dR, W, H, 3 * W, off[0], off[1], dS, dPL, dPR))
                _wait(c)
                assert_bit_equal(g.check(dS, (3, F, fh, fw), f"{scheme} d_stack"), stack, f"foveated {name} {scheme}: the stack")
                assert_bit_equal(g.check(dPL, (F, 3, fh, fw), f"{scheme} d_pyrL"), pl, f"foveated {name} {scheme}: the left pyramid stack")
                assert_bit_equal(g.check(dPR, (F, 3, fh, fw), f"{scheme} d_pyrR"), pr, f"foveated {name} {scheme}: the right pyramid stack")
            finally:
                g.done()


@pytest.mark.parametrize("name", list(FOVEA))
def test_submit_foveated_batch_of_two(lib, orc, name):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    n, nf = 2, 3 * F * fh * fw
    want = [_fov_cold(orc, cfg, j, OFFS2[j], want_pyr=True) for j in range(n)]
    with lib.Context(levels=lv, fovea_levels=F, batch=n) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = [g.image(_pair(W, H, j)[0]) for j in range(n)], [g.image(_pair(W, H, j)[1]) for j in range(n)]
                dS, dPL, dPR = ([g.buf(nf, sh.out()) for _ in range(n)] for _ in range(3))
                c.submit_foveated_batch(0, dL, dR, W, H, 3 * W, OFFS2, dS, dPL, dPR)
                _wait(c)
                for j in range(n):
                    assert_bit_equal(g.check(dS[j], (3, F, fh, fw), f"{scheme} d_stack[{j}]"), want[j][0], f"foveated batch {name} {scheme}: stack {j}")
                    assert_bit_equal(g.check(dPL[j], (F, 3, fh, fw), f"{scheme} d_pyrL[{j}]"), want[j][1], f"foveated batch {name} {scheme}: pyrL {j}")
                    assert_bit_equal(g.check(dPR[j], (F, 3, fh, fw), f"{scheme} d_pyrR[{j}]"), want[j][2], f"foveated batch {name} {scheme}: pyrR {j}")
            finally:
                g.done()


@pytest.mark.parametrize("checked", [False, True], ids=["multi", "multi_checked"])
@pytest.mark.parametrize("name", list(FOVEA))
def test_submit_foveated_multi_two_windows(lib, orc, name, checked):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    L, R = _pair(W, H)
    nf = 3 * F * fh * fw
    want = []
    for off in OFFS2:
        S = _fov_cold(orc, cfg, 0, off)[0]
        if checked:
            B, S = _fov_back(orc, cfg, 0, off), S.copy()
            for k in range(F):
                lvl, m = orc.lr_check(np.ascontiguousarray(S[:, k]), np.ascontiguousarray(B[:, k]), TAU)
                assert 0 < m < fw * fh, "premise: the check fires and spares on every level"
                S[2, k] = lvl[2]
        want.append(S)
    with lib.Context(levels=lv, fovea_levels=F) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = g.image(L), g.image(R)
                dS = [g.buf(nf, sh.out()) for _ in OFFS2]
                if checked:
                    c.submit_foveated_multi_checked(0, dL, dR, W, H, 3 * W, OFFS2, dS, TAU)
                else:
                    c.submit_foveated_multi(0, dL, dR, W, H, 3 * W, OFFS2, dS)
                _wait(c)
                for k in range(2):
                    assert_bit_equal(g.check(dS[k], (3, F, fh, fw), f"{scheme} d_stack[{k}]"), want[k], f"multi {name} checked={checked} {scheme}: window {k}")
            finally:
                g.done()


@pytest.mark.parametrize("form", ["stack", "field"])
@pytest.mark.parametrize("name", list(FOVEA))
def test_submit_foveated_warm(lib, orc, name, form):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    L, R = _pair(W, H)
    s, off, poff, nf = 2, OFFS2[0], OFFS2[1], 3 * F * fh * fw
    pl, pr = _pyr(orc, W, H, 0, lv)
    if form == "stack":
        prior = _fov_cold(orc, cfg, 1, poff)[0]                             # another pair's cold stack at another window
        want = _memo(("warm", cfg), lambda: fs.warm_oracle(orc, None, None, prior, lv, poff, off, s, (pl, pr)))
    else:
        prior = _memo(("warm-prior-field", cfg), lambda: _finite_field(W, H, 8900 + W))
        want = _memo(("warm-field", cfg), lambda: fs.warm_oracle(orc, None, None, prior, lv, None, off, s, (pl, pr), field=True, F=F))
    assert not np.array_equal(want[:, :s + 1].view(np.uint32), _fov_cold(orc, cfg, 0, off)[0][:, :s + 1].view(np.uint32)), "premise: not the cold stack"
    with lib.Context(levels=lv, fovea_levels=F) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = g.image(L), g.image(R)
                dP, dS = g.inp(prior, sh.inp()), g.buf(nf, sh.out())
                if form == "stack":
                    c.submit_foveated_warm(0, [dL], [dR], W, H, 3 * W, [off], [dP], [poff], s, [dS])
                else:
                    c.submit_foveated_warm_field(0, [dL], [dR], W, H, 3 * W, [off], [dP], s, [dS])
                _wait(c)
                assert_bit_equal(g.check(dS, (3, F, fh, fw), f"{scheme} d_stack"), want, f"warm {form} {name} {scheme}")
            finally:
                g.done(f"warm {form} {scheme}")


# ==== after the match =====================================================================================================================

@pytest.mark.parametrize("name", list(FOVEA))
def test_reconstruct_full_and_multi(lib, orc, name):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    rng = np.random.default_rng(8700 + fw)
    stacks = [rm.random_stack(rng, F, fh, fw) for _ in OFFS2]
    want1 = orc.reconstruct_full(stacks[0], W, H, lv, *OFFS2[0])
    want2 = rm.reconstruct_multi(orc, stacks, W, H, lv, OFFS2)
    with lib.Context(levels=lv, fovea_levels=F) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                planes = [g.inp(stacks[0][p], sh.inp()) for p in range(3)]       # three pointers: three buffers
                dO = g.buf(3 * W * H, sh.out())
                c.reconstruct_full(planes[0], planes[1], planes[2], W, H, dO, *OFFS2[0])
                assert_bit_equal(g.check(dO, (3, H, W), f"{scheme} d_out3"), want1, f"reconstruct_full {name} {scheme}")
                dS = [g.inp(st, sh.inp()) for st in stacks]
                dO = g.buf(3 * W * H, sh.out())
                c.reconstruct_full_multi(dS, W, H, dO, OFFS2)
                assert_bit_equal(g.check(dO, (3, H, W), f"{scheme} d_out3 (multi)"), want2, f"reconstruct_full_multi {name} {scheme}")
            finally:
                g.done(f"reconstruct {scheme}")


@pytest.mark.parametrize("size", [QUAD, PAIR_W, ODD], ids=["448x150", "450x152", "451x149"])
def test_warp_planes_warp_right_and_the_residual(lib, orc, size):
    W, H = size
    _residue(size)
    L, R = _pair(W, H)
    d = _finite_field(W, H, 8600 + W)
    d[0, 3, 5], d[1, H - 2, W - 3] = np.nan, np.inf
    L3, R3 = wn.planes(L), wn.planes(R)
    Rw = wn.warp(R3, d[0], d[1])
    sums = wn.residual_sums(L3, Rw, d[2])
    with lib.Context(levels=LEVELS) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL, dR = g.image(L), g.image(R)
                src, dx, dy = g.inp(R3, sh.inp()), g.inp(d[0], sh.inp()), g.inp(d[1], sh.inp())
                dst = g.buf(3 * W * H, sh.out())
                c.warp_planes(src, 3, W, H, dx, dy, dst)
                assert_bit_equal(g.check(dst, (3, H, W), f"{scheme} d_dst"), Rw, f"warp_planes {W}x{H} {scheme}")
                dst = g.buf(3 * W * H, sh.out())
                c.warp_right(dR, W, H, 3 * W, dx, dy, dst)
                assert_bit_equal(g.check(dst, (3, H, W), f"{scheme} d_warp3"), Rw, f"warp_right {W}x{H} {scheme}")
                conf = g.inp(d[2], sh.inp())
                c.photometric_residual(dL, dR, W, H, 3 * W, dx, dy, conf)           # (d_sums: the context's own 8-byte-aligned buffer)
                assert c.last_residual_sums[0].tobytes() == sums.tobytes(), f"residual {W}x{H} {scheme}: {c.last_residual_sums[0]} vs {sums}"
            finally:
                g.done(f"warp {scheme}")


@pytest.mark.parametrize("name", list(FOVEA))
def test_warp_right_fovea_and_the_residual_of_a_stack(lib, orc, name):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    stack, pl, pr = _fov_cold(orc, cfg, 0, OFFS2[0], want_pyr=True)
    warped = np.stack([wn.warp(pr[k], stack[0, k], stack[1, k]) for k in range(F)])
    sums = np.stack([wn.residual_sums(pl[k], warped[k], stack[2, k]) for k in range(F)])
    with lib.Context(levels=lv, fovea_levels=F) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dPL, dPR = g.inp(pl, sh.inp()), g.inp(pr, sh.inp())
                sx, sy, sC = (g.inp(stack[p], sh.inp()) for p in range(3))
                dW = g.buf(F * 3 * fh * fw, sh.out())
                c.warp_right_fovea(dPR, sx, sy, fw, fh, dW)
                assert_bit_equal(g.check(dW, (F, 3, fh, fw), f"{scheme} d_warp"), warped, f"warp_right_fovea {name} {scheme}")
                c.photometric_residual_fovea(dPL, dPR, sx, sy, sC, fw, fh)
                assert c.last_residual_sums.tobytes() == sums.tobytes(), f"residual of the stack {name} {scheme}"
            finally:
                g.done(f"warp fovea {scheme}")


@pytest.mark.parametrize("size", [QUAD, PAIR_W, ODD], ids=["448x150", "450x152", "451x149"])
def test_triangulate_and_point_cloud(lib, orc, size):
    W, H = size
    _residue(size)
    rng = np.random.default_rng(8500 + W)
    dx = rng.normal(-40, 25, (H, W)).astype(np.float32)
    dy = rng.normal(0, 2, (H, W)).astype(np.float32)
    conf = rng.uniform(0, 1, (H, W)).astype(np.float32)
    dx[2, 7], conf[5, 9] = np.nan, np.nan
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    xyz = orc.triangulate(dx, dy, P1, P2A)
    want_cloud = cn.records(xyz, cn.colour_word(rgb), conf=conf, compact=True, min_conf=0.3)
    cap, extra = W * H, 64
    with lib.Context(levels=LEVELS) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                ddx, ddy, dconf, drgb = g.inp(dx, sh.inp()), g.inp(dy, sh.inp()), g.inp(conf, sh.inp()), g.image(rgb)
                dxyz = g.buf(3 * W * H, sh.out())
                c.triangulate(ddx, ddy, W, H, P1, P2A, dxyz)
                assert_bit_equal(g.check(dxyz, (3, H, W), f"{scheme} d_xyz"), xyz, f"triangulate {W}x{H} {scheme}")
                pts = g.image(np.full((cap + extra) * 32, POISON, np.uint8))       # d_points and the count aligned, as the header requires
                cnt = g.image(np.full(1, -7, np.int64))
                n = c.point_cloud(ddx, ddy, dconf, drgb, W, H, 3 * W, P1, P2A, lib.cloud_params(compact=True, min_conf=0.3), pts, cap, cnt)
                raw = c.to_host(pts, ((cap + extra) * 32,), np.uint8)
                assert n == want_cloud.size and (raw[n * 32:] == POISON).all()
                cn.assert_cloud_equal(raw[:n * 32].view(cn.DTYPES[cn.PCL32]), want_cloud, f"point_cloud {W}x{H} {scheme}")
            finally:
                g.done(f"cloud {scheme}")


@pytest.mark.parametrize("name", list(FOVEA))
def test_triangulate_fovea_and_point_cloud_fovea_all(lib, orc, name):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    off = OFFS2[0]
    rng = np.random.default_rng(8400 + fw)
    sx = rng.normal(-20, 10, (F, fh, fw)).astype(np.float32)
    sy = rng.normal(0, 2, (F, fh, fw)).astype(np.float32)
    sC = rng.uniform(0, 1, (F, fh, fw)).astype(np.float32)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    k = 1
    left, upper, scale = lib.fovea_level_mapping(W, H, lv, F, k, off)
    xyz = orc.triangulate_fovea(sx, sy, k, left, upper, scale, P1, P2A)
    want_cloud, want_per = sc.cloud_fovea_all(orc, sx, sy, rgb, off, P1, P2A, stackc=sC, compact=True, min_conf=0.3)
    cap, extra = lib.fovea_cloud_points(W, H, lv, F, off, 1), 64
    with lib.Context(levels=lv, fovea_levels=F) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dsx, dsy, dsc, drgb = g.inp(sx, sh.inp()), g.inp(sy, sh.inp()), g.inp(sC, sh.inp()), g.image(rgb)
                dxyz = g.buf(3 * fw * fh, sh.out())
                c.triangulate_fovea(dsx, dsy, fw, fh, k, left, upper, scale, P1, P2A, dxyz)
                assert_bit_equal(g.check(dxyz, (3, fh, fw), f"{scheme} d_xyz"), xyz, f"triangulate_fovea {name} {scheme}")
                pts = g.image(np.full((cap + extra) * 32, POISON, np.uint8))
                cnt, per = g.image(np.full(1, -7, np.int64)), g.image(np.full(F, -7, np.int64))
                n, got_per = c.point_cloud_fovea_all(dsx, dsy, dsc, W, H, off, drgb, 3 * W, P1, P2A, lib.cloud_params(compact=True, min_conf=0.3),
                                                     pts, cap, cnt, per)
                raw = c.to_host(pts, ((cap + extra) * 32,), np.uint8)
                assert n == want_cloud.size and got_per == want_per and (raw[n * 32:] == POISON).all()
                cn.assert_cloud_equal(raw[:n * 32].view(cn.DTYPES[cn.PCL32]), want_cloud, f"point_cloud_fovea_all {name} {scheme}")
            finally:
                g.done(f"fovea cloud {scheme}")


# ==== the stage entry points: the kernels one by one ======================================================================================

@pytest.mark.parametrize("size", SIZES, ids=[f"{s[0]}x{s[1]}" for s in SIZES])
def test_stage_pyramid_every_level(lib, orc, size):
    W, H = size
    _residue(size)
    L = _pair(W, H)[0]
    pl = _pyr(orc, W, H, 0)[0]
    with lib.Context(levels=LEVELS) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                dL = g.image(L)
                for lev in range(LEVELS):
                    out = g.buf(pl[lev].size, sh.out())
                    c.check(c.lib.ugsm_stage_pyramid(c.handle, dL, W, H, 3 * W, lev, out))
                    assert_bit_equal(g.check(out, pl[lev].shape, f"{scheme} level {lev}"), pl[lev], f"stage_pyramid {W}x{H} {scheme} level {lev}")
            finally:
                g.done()


SMOOTH_CLASSES = dict(CLASS_ENV, small={})          # small: no UGSM_SMALL_MASK -- k_smooth_small where the thresholds pick it
SMOOTH_COMBOS = [(5, 1), (1, 0), (0, 1)]


@pytest.mark.parametrize("cls", list(SMOOTH_CLASSES))
def test_stage_smooth_in_place_every_tile_class(lib, orc, monkeypatch, cls):
    for k, v in SMOOTH_CLASSES[cls].items():
        monkeypatch.setenv(k, v)
    for i, size in enumerate(SIZES):
        W, H = size
        _residue(size)
        plan = lib.plan_level(W, H, alone=True)
        if cls == "small":
            assert plan["smooth_kernel"] == SMALL, f"{cls} {size}: {plan}"
        else:
            assert plan["smooth_kernel"] == FUSED and (plan["smooth_tile_rows"] > 0) == (cls == "112"), f"{cls} {size}: {plan}"
        d = _memo(("smooth-field", size), lambda: field(W, H, 8300 + i))
        exp = _memo(("smooth-exp", size), lambda: expected(orc, d))
        with lib.Context(levels=1, slots=1) as c:
            for scheme in SCHEMES:
                sh, g = Shifts(scheme), Guards(c)
                try:
                    for passes, box in SMOOTH_COMBOS:
                        p = g.buf(d.size, sh.out(), d)
                        c.check(c.lib.ugsm_stage_smooth(c.handle, p, W, H, passes, box))
                        assert_bit_equal(g.check(p, d.shape, f"{cls} {scheme} passes={passes} box={box}"), exp[(passes, box)],
                                         f"stage_smooth {cls} {W}x{H} {scheme} passes={passes} box={box}")
                finally:
                    g.done()


ITERATE = {  # K-cost kernel -> (ugsm_config fields, development overrides, the planned cost_kernel)
    "march": (dict(march_min_pixels=1), {}, MARCH),
    "march4": (dict(small_max_pixels=-1), {"UGSM_MARCH4": "1,2000000000"}, MARCH4),
    "small": ({}, {}, SMALL),
}


@pytest.mark.parametrize("kernel", list(ITERATE))
def test_stage_iterate_every_cost_kernel(lib, orc, monkeypatch, kernel):
    cfg, env, planned = ITERATE[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for i, size in enumerate(SIZES):
        W, H = size
        _residue(size)
        assert lib.plan_level(W, H, alone=True, **cfg)["cost_kernel"] == planned, (kernel, size, lib.plan_level(W, H, alone=True, **cfg))
        pl, pr = (p[0] for p in _pyr(orc, W, H, 0))
        d0 = _memo(("iterate-d0", size), lambda: _finite_field(W, H, 8200 + i))
        want = _memo(("iterate", size), lambda: orc.iterate_level(pl, pr, d0, 6, 5, False, 1, 2)[0])
        with lib.Context(levels=1, **cfg) as c:
            for scheme in SCHEMES:
                sh, g = Shifts(scheme), Guards(c)
                try:
                    dL, dR = g.inp(pl, sh.inp()), g.inp(pr, sh.inp())
                    dd = g.buf(d0.size, sh.out(), d0)
                    c.check(c.lib.ugsm_stage_iterate(c.handle, dL, dR, dd, W, H, 6, 5, 0, 1, 2, None))
                    assert_bit_equal(g.check(dd, d0.shape, f"{kernel} {scheme} d_d3"), want, f"stage_iterate {kernel} {W}x{H} {scheme}")
                finally:
                    g.done(f"stage_iterate {kernel} {scheme}")


@pytest.mark.parametrize("size", [QUAD, PAIR_W, ODD], ids=["448x150", "450x152", "451x149"])
def test_stage_seed_weighted_difference_and_lr_check(lib, orc, size):
    W, H = size
    _residue(size)
    lw, lh = lib.level_dims(W, H, 2)
    src = _finite_field(lw[1], lh[1], 8100 + W)
    seeded = orc.seed(src, W, H)
    crop = orc.seed_fovea(src, W, H, 20, 14)
    a, b = _finite_field(W, H, 8101 + W), _finite_field(W, H, 8102 + W)
    b[0] = -a[0] + np.random.default_rng(8103).normal(0, 0.8, (H, W)).astype(np.float32)
    wd = np.array(orc.weighted_difference(a, b), np.float32)
    checked, marked = orc.lr_check(a, b, TAU)
    assert 0 < marked < W * H
    with lib.Context(levels=LEVELS) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                p, q = g.inp(src, sh.inp()), g.buf(3 * W * H, sh.out())
                c.check(c.lib.ugsm_stage_seed(c.handle, p, lw[1], lh[1], q, W, H, 0, 0, 0, 0))
                assert_bit_equal(g.check(q, (3, H, W), f"{scheme} seed"), seeded, f"stage_seed {W}x{H} {scheme}")
                q = g.buf(src.size, sh.out())
                c.check(c.lib.ugsm_stage_seed(c.handle, p, lw[1], lh[1], q, lw[1], lh[1], W, H, 20, 14))
                assert_bit_equal(g.check(q, src.shape, f"{scheme} fovea seed"), crop, f"stage_seed, fovea form, {W}x{H} {scheme}")
                pa, pb = g.inp(a, sh.inp()), g.inp(b, sh.inp())
                out2 = (C.c_float * 2)()
                c.check(c.lib.ugsm_stage_weighted_difference(c.handle, pa, pb, W, H, out2))
                assert_bit_equal(np.array(out2[:], np.float32), wd, f"stage_weighted_difference {W}x{H} {scheme}")
                left = g.buf(a.size, sh.out(), a)
                n = C.c_longlong(-1)
                c.check(c.lib.ugsm_stage_lr_check(c.handle, left, pb, W, H, C.c_float(TAU), C.byref(n)))
                assert_bit_equal(g.check(left, a.shape, f"{scheme} d_left3"), checked, f"stage_lr_check {W}x{H} {scheme}")
                assert n.value == marked
            finally:
                g.done(f"stages {scheme}")


@pytest.mark.parametrize("size", [QUAD, PAIR_W, ODD], ids=["448x150", "450x152", "451x149"])
def test_stage_restrict_and_prolong_with_a_shifted_source(lib, orc, size):
    W, H = size
    _residue(size)
    lw, lh = lib.level_dims(W, H, LEVELS)
    full = _finite_field(W, H, 8000 + W)
    with lib.Context(levels=LEVELS) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                src = g.inp(full, sh.inp())
                for s in range(LEVELS):
                    dst = g.buf(3 * lw[s] * lh[s], sh.out())
                    c.stage_restrict(src, W, H, s, dst)
                    assert_bit_equal(g.check(dst, (3, lh[s], lw[s]), f"{scheme} restrict to {s}"), sn.restrict_np(full, s, lw[s], lh[s]),
                                     f"stage_restrict {W}x{H} {scheme} level {s}")
                for e in range(LEVELS):
                    st = _finite_field(lw[e], lh[e], 8001 + e)
                    psrc, dst = g.inp(st, sh.inp()), g.buf(3 * W * H, sh.out())
                    c.stage_prolong(psrc, W, H, e, dst)
                    assert_bit_equal(g.check(dst, (3, H, W), f"{scheme} prolong from {e}"), co.prolong_np(st, (lw[:e + 1], lh[:e + 1])),
                                     f"stage_prolong {W}x{H} {scheme} level {e}")
            finally:
                g.done(f"restrict / prolong {scheme}")


@pytest.mark.parametrize("name", list(FOVEA))
def test_stage_warm_stack_with_a_shifted_source(lib, orc, name):
    cfg, (fw, fh) = _fovea(lib, name)
    W, H, lv, F = cfg
    poff, off = OFFS2[1], OFFS2[0]
    prior = fs.special_stack(F, fh, fw, 7900 + fw)
    want = fs.start_fields(orc, prior, W, H, lv, poff, off, 0)
    with lib.Context(levels=lv, fovea_levels=F) as c:
        for scheme in SCHEMES:
            sh, g = Shifts(scheme), Guards(c)
            try:
                src = g.inp(prior, sh.inp())
                for s in (0, F - 1):
                    dst = g.buf(prior.size, sh.out())
                    c.stage_warm_stack(src, W, H, poff, off, s, dst)
                    got = g.check(dst, prior.shape, f"{scheme} start level {s}")
                    for k in range(s, F):
                        assert_bit_equal(got[:, k], want[k], f"stage_warm_stack {name} {scheme}, start level {s}, level {k}")
                    assert (np.ascontiguousarray(got[:, :s]).view(np.uint8) == POISON).all(), f"start level {s}: a row block below it was written"
            finally:
                g.done(f"warm stack {scheme}")
