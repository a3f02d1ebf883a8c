"""The merged cloud of several fovea windows of one pair (ugsm_fovea_multi_cloud_points / ugsm_point_cloud_fovea_multi) without a GPU:
declarations and exports, the pinned dense sizes, n == 1 against ugsm_fovea_cloud_points, the kept footprints leaving no hole, the CPU
restatement (tests/multi_cloud_np.py) on a hand-made pair of windows, and the refusal of a call without a context (the argument
checks themselves need a live context: tests/test_gpu_multi_cloud.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cloud_np as cn
import multi_cloud_np as mn
import stack_cloud_np as sn
from conftest import ROOT
from test_stack_cloud_host import OFFSETS, TABLE, _NamingOracle, _intervals
from test_stack_cloud_host import bad_argument_cases as stack_cases

NEW = ["ugsm_fovea_multi_cloud_points", "ugsm_point_cloud_fovea_multi"]

# W, H, F, the windows' offsets, dense points, per entry (level-major), dense points at sampling 3: evaluated from the rule's text with a
# numpy model in float32
CASES = [
    (40, 30, 2, [(-100, -100), (100, 100)], 1110, [396, 588, 126], 131),
    (160, 120, 4, [(0, 0), (30, -20), (30, -20), (-500, 500)], 10428, [1726, 0, 2255, 2255, 535, 0, 909, 953, 206, 0, 730, 528, 331], 1255),
    (320, 240, 4, [(-60, 40), (0, 0), (25, 10)], 35189, [6850, 2970, 9408, 3092, 1462, 2827, 2276, 924, 2874, 2506], 4097),
    (160, 120, 7, [(0, 0), (23, -17)], 1684, None, None),
    (333, 251, 3, [(0, 0), (-40, 33), (90, 0), (91, 1), (-400, -400)], 67594, [33, 13277, 166, 20750, 20750, 0, 4029, 69, 2914, 3360, 2246], None),
]
LEVELS = {2: 2, 3: 8, 4: 9, 7: 14}    # a context's `levels` for each F of the cases (only F enters the cloud)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_multi_cloud_symbols_are_declared_and_exported_by_both_libraries(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().ugsm_abi_version() == 6


@pytest.mark.parametrize("W,H,F,offsets,points,per,points3", CASES)
def test_pinned_dense_sizes(lib, W, H, F, offsets, points, per, points3):
    got = lib.fovea_multi_cloud_points(W, H, LEVELS[F], F, offsets, 1, per_entry=True)
    mine = mn.fovea_multi_cloud_points(W, H, F, offsets)
    assert got == mine and got[0] == points and len(got[1]) == (F - 1) * len(offsets) + 1 and sum(got[1]) == points
    if per is not None:
        assert got[1] == per
    for s in (2, 3, 7):
        assert lib.fovea_multi_cloud_points(W, H, LEVELS[F], F, offsets, s, per_entry=True) == mn.fovea_multi_cloud_points(W, H, F, offsets, s), s
    if points3 is not None:
        assert lib.fovea_multi_cloud_points(W, H, LEVELS[F], F, offsets, 3) == points3
    assert lib.fovea_multi_cloud_points(W, H, LEVELS[F], F, offsets) == points     # (per_entry NULL)
    n = len(offsets)
    zero = (C.c_int * n)()
    centred = lib.load().ugsm_fovea_multi_cloud_points(W, H, LEVELS[F], F, n, None, None, 1, None)     # NULL offsets: all centred
    assert centred == lib.load().ugsm_fovea_multi_cloud_points(W, H, LEVELS[F], F, n, zero, zero, 1, None) == \
        mn.fovea_multi_cloud_points(W, H, F, [(0, 0)] * n)[0]


def test_the_two_window_case_in_words(lib):
    """40 x 30, F = 2: the windows clamp to origins (0, 0) and (12, 9); window 0 loses the 16 x 12 pixels window 1 holds."""
    W, H, F, offsets = CASES[0][:4]
    assert [sn.level_mapping(W, H, F, 0, o)[:2] for o in offsets] == [(0, 0), (12, 9)]
    out = mn.left_out(W, H, F, offsets, 0, 0)
    assert int(out.sum()) == 16 * 12 and out[9:, 12:].all()
    assert not mn.left_out(W, H, F, offsets, 1, 0).any()


def test_one_window_is_the_stack_cloud(lib):
    for (W, H, levels, F, *_rest) in TABLE:
        for off in OFFSETS:
            for s in (1, 3):
                assert lib.fovea_multi_cloud_points(W, H, levels, F, [off], s, per_entry=True) == \
                    lib.fovea_cloud_points(W, H, levels, F, off, s, per_level=True), (W, H, off, s)


def test_size_refusals(lib):
    f = lib.fovea_multi_cloud_points
    assert f(640, 480, 14, 7, [(0, 0)] * 16) > 0
    for bad in [dict(W=0), dict(H=0), dict(sampling=0), dict(sampling=-1), dict(F=1), dict(F=15), dict(levels=33), dict(W=8, H=8),
                dict(offsets=[]), dict(offsets=[(0, 0)] * 17)]:
        a = dict(dict(W=640, H=480, levels=14, F=7, offsets=[(0, 0), (5, 5)], sampling=1), **bad)
        assert f(a["W"], a["H"], a["levels"], a["F"], a["offsets"], a["sampling"]) == -1, bad


def _cell_owner(n, m, sc, cells):
    """For each 1/4-pixel cell centre along an axis: the pixel of a level whose footprint holds it (-1: none)."""
    lo, hi = _intervals(n, m, sc)
    centre = (np.arange(cells) + 0.5) / 4.0
    idx = np.searchsorted(lo, centre, side="right") - 1
    ok = (idx >= 0) & (centre < hi[np.clip(idx, 0, n - 1)])
    return np.where(ok, idx, -1)


@pytest.mark.parametrize("W,H,F,offsets", [c[:4] for c in CASES])
def test_kept_footprints_leave_no_hole(lib, W, H, F, offsets):
    """The kept pixels' footprints, rasterised on a 1/4-pixel grid over the extent of level F-1: no cell is uncovered.  Neighbours of one
    level abut as in test_stack_cloud_host._intervals."""
    fw, fh = sn.fovea_dims(W, H, F)
    top = sn.level_mapping(W, H, F, F - 1)
    ex, ey = (int(np.floor(_intervals(n, m, top[2])[1][-1] * 4)) for n, m in ((fw, top[0]), (fh, top[1])))
    seen = np.zeros((ey, ex), bool)
    for j, k in mn.entries(F, len(offsets)):
        left, upper, sc = sn.level_mapping(W, H, F, k, offsets[j])
        cx, cy = _cell_owner(fw, left, sc, ex), _cell_owner(fh, upper, sc, ey)
        kept = ~mn.left_out(W, H, F, offsets, j, k)
        seen |= kept[np.clip(cy, 0, None)[:, None], np.clip(cx, 0, None)[None, :]] & (cy >= 0)[:, None] & (cx >= 0)[None, :]
    assert seen.all(), f"{int((~seen).sum())} of the 1/4-pixel cells are uncovered"


def test_restatement_on_two_windows_of_a_two_level_stack(lib):
    """40 x 30, two levels, windows at (0, 0) and (12, 9), 28 x 21 each.  Entry 0 = level 0 of window 0 without columns 12 .. 27 x rows
    9 .. 20 (inside window 1); entry 1 = level 0 of window 1, whole; entry 2 = level 1 (scale 1.414) without the pixels inside window 0
    -- (ii + 1) * 1.414 <= 28 and (jj + 1) * 1.414 <= 21: ii <= 18, jj <= 13 -- or inside window 1 -- 12 <= ii * 1.414,
    (ii + 1) * 1.414 <= 40, 9 <= jj * 1.414, (jj + 1) * 1.414 <= 30: ii >= 9, jj >= 7."""
    W, H, F, offsets = CASES[0][:4]
    stack = np.zeros((3, F, 21, 28), np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[..., 0], rgb[..., 2] = np.arange(H)[:, None], np.arange(W)[None, :]
    P = np.eye(3, 4)
    rec, per = mn.cloud_fovea_multi(_NamingOracle, [stack, stack], rgb, offsets, P, P)
    assert per == [396, 588, 126] and rec.size == 1110
    assert lib.fovea_multi_cloud_points(W, H, 2, F, offsets, per_entry=True) == (1110, per)
    exp = [100 * i + j for i in range(28) for j in range(21) if not (i >= 12 and j >= 9)]
    exp += [100 * i + j for i in range(28) for j in range(21)]
    exp += [10000 + 100 * i + j for i in range(28) for j in range(21) if not ((i <= 18 and j <= 13) or (i >= 9 and j >= 7))]
    assert rec["x"].tolist() == exp
    # the colours are read at the mapped pixels: window 0's (0, 0) at (0, 0), window 1's (0, 0) at (12, 9) and its (2, 1) at (14, 10);
    # level 1's pixel (27, 0) at ((int)(27 * sqrt 2), 0)
    assert rec["rgb"][0] == 0 and rec["rgb"][396] == (9 << 16) | 12 and rec["rgb"][396 + 2 * 21 + 1] == (10 << 16) | 14
    assert rec["rgb"][396 + 588 + exp[396 + 588:].index(10000 + 2700)] == int(27 * 2 ** 0.5)
    # sampling 3
    rec3, per3 = mn.cloud_fovea_multi(_NamingOracle, [stack, stack], rgb, offsets, P, P, s=3, fmt=cn.XYZRGB16)
    cols3, rows3 = list(range(0, 28, 3)), list(range(0, 21, 3))
    exp3 = [100 * i + j for i in cols3 for j in rows3 if not (i >= 12 and j >= 9)] + [100 * i + j for i in cols3 for j in rows3]
    exp3 += [10000 + 100 * i + j for i in cols3 for j in rows3 if not ((i <= 18 and j <= 13) or (i >= 9 and j >= 7))]
    assert rec3["x"].tolist() == exp3 and per3 == [46, 70, 15] and sum(per3) == 131
    # compaction: a low and a NaN confidence drop their pixels; left-out pixels stay out
    s0, s1 = stack.copy(), stack.copy()
    s0[2], s1[2] = 0.9, 0.9
    s0[2, 0, 2, 1], s0[2, 0, 15, 20], s1[2, 0, 0, 0], s0[2, 1, 0, 27] = 0.1, 0.1, np.nan, 0.1   # (the second is left out anyway)
    s1[2, 1] = 0.0                                                                          # (level F-1 is read from stack 0 alone)
    recc, perc = mn.cloud_fovea_multi(_NamingOracle, [s0, s1], rgb, offsets, P, P, compact=True, min_conf=0.5)
    assert perc == [395, 587, 125]
    gone = {0: [102], 1: [0], 2: [10000 + 2700]}
    want = [v for e, part in enumerate((exp[:396], exp[396:984], exp[984:])) for v in part if v not in gone[e]]
    assert recc["x"].tolist() == want
    assert mn.cloud_fovea_multi(_NamingOracle, [s0, s1], rgb, offsets, P, P, compact=True, z_min=3.0)[1] == [0, 0, 0]


def _call(lib, ctx=None, **over):
    """One ugsm_point_cloud_fovea_multi call with plausible (fake, never dereferenced) device pointers, `over` replacing arguments:
    test_stack_cloud_host._call's names, dx / dy standing for the first / second stack, `stacks` for the array itself."""
    P = (C.c_double * 12)(*range(12))
    a = dict(dx=0x10000, dy=0x20000, rgb=0x40000, W=640, H=480, stride=1920, P1=P, P2=P, p=lib.cloud_params(), points=0x50000, cap=100,
             count=0x60000, entry_counts=0x70000, n=2, stacks=True)
    a.update(over)
    if "level_counts" in over:
        a["entry_counts"] = over["level_counts"]
    p = C.byref(a["p"]) if a["p"] is not None else None
    stacks = (C.c_void_p * 16)(a["dx"], a["dy"], *([0x30000] * 14)) if a["stacks"] else None
    return lib.load().ugsm_point_cloud_fovea_multi(ctx, 0, a["n"], stacks, a["W"], a["H"], None, None, a["rgb"], a["stride"], a["P1"], a["P2"],
                                                   p, a["points"], a["cap"], a["count"], a["entry_counts"])


def bad_argument_cases(lib):
    """Every argument refusal of ugsm_point_cloud_fovea_multi (name, overrides): ugsm_point_cloud_fovea_all's -- but for its null
    confidence plane, an argument this call does not have: a stack carries its own -- and n outside 1 .. 16, a null array, a null entry;
    shared with the GPU test, which makes them on a live context."""
    return [c for c in stack_cases(lib) if "conf" not in c[1]] + [
        ("n 0", dict(n=0)), ("n 17", dict(n=17)), ("n < 0", dict(n=-1)), ("no array", dict(stacks=False)),
        ("entry_counts misaligned", dict(entry_counts=0x70004))]


def test_null_context_and_bad_arguments_are_refused_without_a_device(lib):
    """Without a device there is no context, so every call here is refused for its null context, whatever else it carries: this shows
    that the entry point takes the argument list and answers before it touches anything.  Each argument check on its own is exercised by
    tests/test_gpu_multi_cloud.py on a live context, with the cases listed above."""
    assert _call(lib) == lib.UGSM_ERR_BAD_ARG           # (no context)
    assert _call(lib, entry_counts=None) == lib.UGSM_ERR_BAD_ARG
    for name, over in bad_argument_cases(lib):
        assert _call(lib, **over) == lib.UGSM_ERR_BAD_ARG, name
