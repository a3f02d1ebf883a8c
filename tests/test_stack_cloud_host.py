"""The merged cloud of the whole fovea stack (ugsm_fovea_level_mapping / ugsm_fovea_cloud_points / ugsm_point_cloud_fovea_all) without a
GPU: declarations and exports, the mapping against ugsm_fovea_mapping, the pinned dense sizes, the properties of the coverage rule,
argument refusals, and the CPU restatement (tests/stack_cloud_np.py) on a hand-made two-level stack."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cloud_np as cn
import stack_cloud_np as sn
from conftest import ROOT

NEW = ["ugsm_fovea_level_mapping", "ugsm_fovea_cloud_points", "ugsm_point_cloud_fovea_all"]

# W, H, levels, F, offset, dense points, F * fovW * fovH, covered columns and rows at level 1: evaluated from the rule's text in float32
TABLE = [
    (4928, 3264, 14, 7, (0, 0), 1005221, 1752135, (434, 286)),
    (1920, 1080, 14, 7, (0, 0), 129430, 224182, (168, 94)),
    (640, 480, 14, 7, (0, 0), 18859, 32074, (54, 40)),
    (160, 120, 14, 7, (0, 0), 1078, 1638, (12, 8)),
    (320, 240, 9, 4, (0, 0), 23924, 37632, (78, 58)),
    (1920, 1080, 14, 7, (400, -250), 129766, None, None),
]
OFFSETS = [(0, 0), (400, -250), (-5000, 5000)]   # centred, the table's, and one that clamps every window into a corner


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_stack_cloud_symbols_are_declared_and_exported_by_both_libraries(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().ugsm_abi_version() == 6


@pytest.mark.parametrize("W,H", [(4928, 3264), (1920, 1080), (640, 480), (160, 120)])
def test_level_mapping_is_fovea_mapping_for_seven_centred_levels(lib, W, H):
    for k in range(7):
        got = lib.fovea_level_mapping(W, H, 14, 7, k)
        ref = lib.fovea_mapping(W, H, k, 0)
        assert got[:2] == ref[:2] and np.float32(got[2]).view(np.uint32) == np.float32(ref[2]).view(np.uint32), (k, got, ref)
        mine = sn.level_mapping(W, H, 7, k)
        assert mine[:2] == got[:2] and mine[2].view(np.uint32) == np.float32(got[2]).view(np.uint32), (k, mine, got)


def test_level_mapping_with_offsets_and_other_level_counts_matches_the_restatement(lib):
    for (W, H, levels, F) in [(1920, 1080, 14, 7), (320, 240, 9, 4), (4928, 3264, 14, 7), (640, 480, 5, 2), (640, 480, 12, 12)]:
        for off in OFFSETS + [(37, 11), (-123, 77)]:
            for k in range(F):
                got, mine = lib.fovea_level_mapping(W, H, levels, F, k, off), sn.level_mapping(W, H, F, k, off)
                assert got[:2] == mine[:2] and np.float32(got[2]).view(np.uint32) == mine[2].view(np.uint32), (W, H, F, off, k, got, mine)
            assert lib.fovea_level_mapping(W, H, levels, F, F - 1, off)[:2] == (0, 0)   # the coarsest level is the whole frame


def test_level_mapping_refusals(lib):
    so = lib.load()
    l, u, sc = C.c_int(), C.c_int(), C.c_float()
    ok = dict(W=640, H=480, levels=14, F=7, ox=0, oy=0, k=3, l=C.byref(l), u=C.byref(u), sc=C.byref(sc))

    def call(**over):
        a = dict(ok, **over)
        return so.ugsm_fovea_level_mapping(a["W"], a["H"], a["levels"], a["F"], a["ox"], a["oy"], a["k"], a["l"], a["u"], a["sc"])
    assert call() == lib.UGSM_OK
    for name, over in [("left NULL", dict(l=None)), ("upper NULL", dict(u=None)), ("scale NULL", dict(sc=None)), ("F 1", dict(F=1)),
                       ("F 0", dict(F=0)), ("F > levels", dict(F=8, levels=7)), ("k < 0", dict(k=-1)), ("k == F", dict(k=7)),
                       ("W 0", dict(W=0)), ("H 0", dict(H=0)), ("levels above the maximum", dict(levels=lib.UGSM_MAX_LEVELS + 1)),
                       ("too small for F levels", dict(W=8, H=8)), ("H above a grid's rows", dict(H=70000))]:
        assert call(**over) == lib.UGSM_ERR_BAD_ARG, name


@pytest.mark.parametrize("W,H,levels,F,off,points,total,cov1", TABLE)
def test_dense_points_of_the_table(lib, W, H, levels, F, off, points, total, cov1):
    n, per = lib.fovea_cloud_points(W, H, levels, F, off, 1, per_level=True)
    fw, fh = sn.fovea_dims(W, H, F)
    assert n == points
    assert sum(per) == n and len(per) == F and per[0] == fw * fh
    assert (n, per) == sn.fovea_cloud_points(W, H, F, off)
    if total is not None:
        assert F * fw * fh == total
        cols, rows = sn.covered(W, H, F, 1, off)
        assert (int(cols.sum()), int(rows.sum())) == cov1
        assert per[1] == fw * fh - cov1[0] * cov1[1]
    assert lib.fovea_cloud_points(W, H, levels, F, off) == n    # (per_level NULL)
    assert lib.load().ugsm_fovea_cloud_points(W, H, levels, F, off[0], off[1], 1, None) == n


def test_sampled_sizes_match_the_restatement(lib):
    for (W, H, levels, F, *_rest) in TABLE[:5]:
        for off in OFFSETS:
            for s in (2, 3, 7):
                assert lib.fovea_cloud_points(W, H, levels, F, off, s, per_level=True) == sn.fovea_cloud_points(W, H, F, off, s), (W, H, off, s)


def test_cloud_points_refusals(lib):
    f = lib.fovea_cloud_points
    assert f(640, 480, 14, 7) > 0
    for bad in [dict(W=0), dict(H=0), dict(sampling=0), dict(sampling=-1), dict(fovea_levels=1), dict(fovea_levels=15), dict(levels=33),
                dict(W=8, H=8)]:
        a = dict(dict(W=640, H=480, levels=14, fovea_levels=7, sampling=1), **bad)
        assert f(a["W"], a["H"], a["levels"], a["fovea_levels"], (0, 0), a["sampling"]) == -1, bad


def _intervals(n, m, sc):
    """Where each pixel of a level starts and ends along an axis.  Neighbours of one level abut by construction: a pixel ends where the
    next one starts, though x1[i] + sc and x1[i + 1] are rounded separately and may differ in the last bit (the end is the larger)."""
    x1 = np.float32(m) + np.arange(n, dtype=np.float32) * np.float32(sc)
    end = x1 + np.float32(sc)
    end[:-1] = np.maximum(end[:-1], x1[1:])
    return x1.astype(np.float64), end.astype(np.float64)


@pytest.mark.parametrize("W,H,levels,F", [t[:4] for t in TABLE[:5]])
def test_covered_sets_are_contiguous_and_the_kept_footprints_leave_no_gap(lib, W, H, levels, F):
    """Per level the covered columns are one interval and the covered rows another; along either axis the footprints of level 0's
    pixels and of the uncovered columns (rows) of the levels above tile the whole frame's extent without a gap.  The library's
    per-level sizes are those of these very sets."""
    fw, fh = sn.fovea_dims(W, H, F)
    for off in OFFSETS:
        per = lib.fovea_cloud_points(W, H, levels, F, off, 1, per_level=True)[1]
        assert per == [fw * fh - int(c.sum()) * int(r.sum()) for c, r in (sn.covered(W, H, F, k, off) for k in range(F))], off
        for axis, n in ((0, fw), (1, fh)):
            spans = []
            for k in range(F):
                cov = sn.covered(W, H, F, k, off)[axis]
                idx = np.flatnonzero(cov)
                assert idx.size == 0 or (idx[-1] - idx[0] + 1 == idx.size), (off, axis, k)
                assert k == 0 or 0 < idx.size < n, (off, axis, k)     # something is covered, and never a whole level
                m, sc = sn.level_mapping(W, H, F, k, off)[axis], sn.scale_of(k)
                lo, hi = _intervals(n, m, sc)
                spans += [(a, b) for a, b, c in zip(lo, hi, cov) if not c]
            spans.sort()
            m, sc = sn.level_mapping(W, H, F, F - 1, off)[axis], sn.scale_of(F - 1)
            lo, hi = _intervals(n, m, sc)
            assert spans[0][0] <= lo[0]
            reach = spans[0][1]
            for a, b in spans[1:]:
                assert a <= reach, f"a gap between {reach} and {a} (offset {off}, axis {axis})"
                reach = max(reach, b)
            assert reach >= hi[-1]


def _call(lib, ctx=None, **over):
    """One ugsm_point_cloud_fovea_all call with plausible (fake, never dereferenced) device pointers, `over` replacing arguments."""
    P = (C.c_double * 12)(*range(12))
    a = dict(dx=0x10000, dy=0x20000, conf=0x30000, rgb=0x40000, W=640, H=480, ox=0, oy=0, stride=1920, P1=P, P2=P, p=lib.cloud_params(),
             points=0x50000, cap=100, count=0x60000, level_counts=0x70000)
    a.update(over)
    p = C.byref(a["p"]) if a["p"] is not None else None
    return lib.load().ugsm_point_cloud_fovea_all(ctx, 0, a["dx"], a["dy"], a["conf"], a["W"], a["H"], a["ox"], a["oy"], a["rgb"], a["stride"],
                                                 a["P1"], a["P2"], p, a["points"], a["cap"], a["count"], a["level_counts"])


def bad_argument_cases(lib):
    """Every argument refusal of ugsm_point_cloud_fovea_all (name, overrides): ugsm_point_cloud_fovea's and the misaligned
    d_level_counts; shared with the GPU test, which makes them on a live context (fovea_levels < 2 needs a context of its own)."""
    from test_cloud_host import bad_argument_cases as cloud_cases
    return cloud_cases(lib) + [("level_counts misaligned", dict(level_counts=0x70004))]


def test_null_context_and_bad_arguments_are_refused_without_a_device(lib):
    assert _call(lib) == lib.UGSM_ERR_BAD_ARG           # (no context)
    assert _call(lib, level_counts=None) == lib.UGSM_ERR_BAD_ARG
    for name, over in bad_argument_cases(lib):
        assert _call(lib, **over) == lib.UGSM_ERR_BAD_ARG, name


# ---- the restatement on a hand-made two-level stack -------------------------------------------------------------------------------

class _NamingOracle:
    """Stands in for the CPU oracle: X names the pixel (10000 * level + 100 * ii + jj), Y = -1, Z = 2."""

    @staticmethod
    def triangulate_fovea(stackx, stacky, src_level, left, upper, scale, P1, P2):
        _, fh, fw = stackx.shape
        jj, ii = np.mgrid[0:fh, 0:fw]
        X = (10000 * src_level + 100 * ii + jj).astype(np.float32)
        return np.stack([X, np.full_like(X, -1), np.full_like(X, 2)])


def test_restatement_on_a_two_level_stack(lib):
    """40 x 30, two levels: the window is 28 x 21 at (6, 5) of level 0, level 1 is the whole frame at scale sqrt(2).  Level 1's pixel
    (ii, jj) is covered when 6 <= ii * 1.414 and (ii + 1) * 1.414 <= 34, and 5 <= jj * 1.414 and (jj + 1) * 1.414 <= 26: columns
    5 .. 23 (5 * 1.414 = 7.07, 24 * 1.414 = 33.94) and rows 4 .. 17 (4 * 1.414 = 5.66, 18 * 1.414 = 25.46)."""
    W, H, F = 40, 30, 2
    assert sn.fovea_dims(W, H, F) == (28, 21)
    assert sn.level_mapping(W, H, F, 0) == (6, 5, np.float32(1.0))
    l1 = sn.level_mapping(W, H, F, 1)
    assert l1[:2] == (0, 0) and abs(float(l1[2]) - 2 ** 0.5) < 1e-6
    cols, rows = sn.covered(W, H, F, 1)
    assert np.flatnonzero(cols).tolist() == list(range(5, 24)) and np.flatnonzero(rows).tolist() == list(range(4, 18))
    assert not sn.covered(W, H, F, 0)[0].any() and not sn.covered(W, H, F, 0)[1].any()
    stack = np.zeros((F, 21, 28), np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[..., 0], rgb[..., 2] = np.arange(H)[:, None], np.arange(W)[None, :]
    P = np.eye(3, 4)
    rec, per = sn.cloud_fovea_all(_NamingOracle, stack, stack, rgb, (0, 0), P, P)
    assert per == [28 * 21, 28 * 21 - 19 * 14] and rec.size == sum(per) == sn.fovea_cloud_points(W, H, F)[0]
    assert lib.fovea_cloud_points(W, H, 2, F, per_level=True) == (sum(per), per)
    assert [lib.fovea_level_mapping(W, H, 2, F, k)[:2] for k in range(F)] == [(6, 5), (0, 0)]
    # level, then column, then row
    exp = [100 * i + j for i in range(28) for j in range(21)]
    exp += [10000 + 100 * i + j for i in range(28) for j in range(21) if not (5 <= i <= 23 and 4 <= j <= 17)]
    assert rec["x"].tolist() == exp
    # the colour of level 0's pixel (ii, jj) is the image's at (6 + ii, 5 + jj); level 1's at ((int)(ii * sqrt 2), (int)(jj * sqrt 2))
    assert rec["rgb"][0] == (5 << 16) | 6 and rec["rgb"][21 + 2] == (7 << 16) | 7
    k = exp.index(10000 + 100 * 27 + 20)
    assert rec["rgb"][k] == (int(20 * 2 ** 0.5) << 16) | int(27 * 2 ** 0.5)
    # sampling 3: pixels 0, 3, 6, ..; the covered sampled columns are 6 .. 21, the rows 6 .. 15
    rec3, per3 = sn.cloud_fovea_all(_NamingOracle, stack, stack, rgb, (0, 0), P, P, s=3, fmt=cn.XYZRGB16)
    cols3, rows3 = list(range(0, 28, 3)), list(range(0, 21, 3))
    exp3 = [100 * i + j for i in cols3 for j in rows3]
    exp3 += [10000 + 100 * i + j for i in cols3 for j in rows3 if not (5 <= i <= 23 and 4 <= j <= 17)]
    assert rec3["x"].tolist() == exp3 and per3 == [70, 70 - 6 * 4] and (sum(per3), per3) == sn.fovea_cloud_points(W, H, F, s=3)
    # compaction: a confidence below the threshold and a NaN confidence drop their pixels, covered pixels stay out
    conf = np.full((F, 21, 28), 0.9, np.float32)
    conf[0, 2, 1], conf[1, 0, 0], conf[1, 10, 10] = 0.1, np.nan, 0.1    # (the last is covered anyway)
    recc, perc = sn.cloud_fovea_all(_NamingOracle, stack, stack, rgb, (0, 0), P, P, stackc=conf, compact=True, min_conf=0.5)
    assert perc == [per[0] - 1, per[1] - 1]
    assert recc["x"].tolist() == [v for v in exp if v not in (102, 10000)]
    assert sn.cloud_fovea_all(_NamingOracle, stack, stack, rgb, (0, 0), P, P, compact=True, z_min=3.0)[1] == [0, 0]
