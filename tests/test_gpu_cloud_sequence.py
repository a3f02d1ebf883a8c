"""Every slot-level cloud form in a row on ONE context and ONE slot, nothing waited for in between: the forms share the slot's count buffer
(csrc/ugsm_cloud.cpp, cloud_begin), which is sized per call over 1, F or E virtual grids -- regrown where it is too small, reused where it
is larger than the call needs, its totals zeroed at another place each time.  Every cloud against the CPU restatements the forms' own
tests use (tests/cloud_np.py, resize_np.py, stack_cloud_np.py, multi_cloud_np.py): byte for byte, a NaN X, Y or Z equal to any NaN."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import multi_cloud_np as mn
import resize_np as rn
import stack_cloud_np as sn
from test_gpu_cloud import P1, P2A, _inputs, _poisoned, _read
from test_gpu_multi_cloud import _per_entry, _random_stacks, _z_window
from test_multi_cloud_host import CASES, LEVELS

pytestmark = pytest.mark.gpu

W, H, F = CASES[2][:3]            # 320 x 240, four fovea levels
OFFSETS = CASES[2][3][:2]         # two windows
SW, SH = 33, 7                    # the first cloud: a count buffer of a few words, which every later call outgrows
FACTOR = 0.3
EXTRA = 64                        # records of poison behind every cloud


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def _z_range(z):
    return tuple(float(np.percentile(z[np.isfinite(z)], q)) for q in (10, 90))


def _level_cloud(orc, stack, k, mapping, rgb, und, s, fmt, **kw):
    """cloud_np.cloud_fovea for level k of a stack, X, Y, Z of the pixels whose integer conversion C leaves undefined taken from the dense
    records `und` ugsm_point_cloud_fovea wrote (stack_cloud_np's note): the sampled planes patched, then cloud_np.records' compaction."""
    fh, fw = stack[0][k].shape
    wc, hc = -(-fw // s), -(-fh // s)
    xyz = np.array(orc.triangulate_fovea(stack[0], stack[1], k, *mapping, P1, P2A), np.float32)[:, ::s, ::s].copy()
    undef = sn.undefined_conversion(stack[0], stack[1], k, s).reshape(wc, hc).T
    for i, name in enumerate("xyz"):
        xyz[i][undef] = und[name].reshape(wc, hc).T[undef]
    cx, cy, _ = cn.fovea_colour_at(rgb.shape[1], rgb.shape[0], fw, fh, *mapping)
    word = cn.colour_word(rgb)[np.ix_(cy, cx)][::s, ::s]
    return cn.records(xyz, word, fmt=fmt, conf=stack[2][k][::s, ::s], compact=True, **kw)


@pytest.mark.parametrize("s,fmt", [(1, cn.PCL32), (3, cn.XYZRGB16)])
def test_every_form_in_a_row_on_one_slot(lib, orc, s, fmt):
    """33 x 7 full frame; the merged cloud of two windows of 320 x 240; window 0's whole stack; its level 1; 320 x 240 planes; the same
    resized by 0.3 (the resized forms take no sampling: 1 there); the merged cloud again.  All compact, with a confidence threshold and a
    Z window; each into its own poisoned buffer and count words; one ugsm_wait at the end.  The second merged cloud equals the first."""
    rng = np.random.Generator(np.random.PCG64(1000 + s))
    n, E, item = len(OFFSETS), (F - 1) * len(OFFSETS) + 1, cn.DTYPES[fmt].itemsize
    stacks, rgb = _random_stacks(rng, W, H, F, n)
    small, planes = _inputs(rng, SW, SH), _inputs(rng, W, H)
    fw, fh = sn.fovea_dims(W, H, F)
    mapping = sn.level_mapping(W, H, F, 1, OFFSETS[0])
    dp = C.POINTER(C.c_double)
    p1, p2 = (np.ascontiguousarray(P, np.float64).reshape(12) for P in (P1, P2A))
    pp = (p1.ctypes.data_as(dp), p2.ctypes.data_as(dp))

    # the dense records of every entry, for the pixels the restatements take from them: on a context of its own (the one under test stays fresh)
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        und = _per_entry(c, lib, d_stacks, d_rgb, W, H, OFFSETS, fmt, s)
        for p in d_stacks + [d_rgb]:
            c.free(p)
    und_stack = [und[k * n] for k in range(F - 1)] + [und[E - 1]]    # (window 0's levels among the entries, level-major)

    # what every call must write
    kw_f = dict(min_conf=0.3, **dict(zip(("z_min", "z_max"), _z_window(orc, stacks, W, H, F, OFFSETS))))
    kw_s = dict(min_conf=0.3, **dict(zip(("z_min", "z_max"), _z_range(orc.triangulate(small[0], small[1], P1, P2A)[2]))))
    kw_p = dict(min_conf=0.3, **dict(zip(("z_min", "z_max"), _z_range(orc.triangulate(planes[0], planes[1], P1, P2A)[2]))))
    exp_multi, per_multi = mn.cloud_fovea_multi(orc, stacks, rgb, OFFSETS, P1, P2A, s=s, fmt=fmt, compact=True, undefined=und, **kw_f)
    exp_stack, per_stack = sn.cloud_fovea_all(orc, stacks[0][0], stacks[0][1], rgb, OFFSETS[0], P1, P2A, stackc=stacks[0][2], s=s, fmt=fmt,
                                              compact=True, undefined=und_stack, **kw_f)
    expected = [cn.cloud(orc, small[0], small[1], small[3], P1, P2A, conf=small[2], s=s, fmt=fmt, compact=True, **kw_s),
                exp_multi, exp_stack, _level_cloud(orc, stacks[0], 1, mapping, rgb, und[n], s, fmt, **kw_f),
                cn.cloud(orc, planes[0], planes[1], planes[3], P1, P2A, conf=planes[2], s=s, fmt=fmt, compact=True, **kw_p),
                rn.resized_cloud(orc, planes[0], planes[1], planes[3], P1, P2A, FACTOR, conf=planes[2], fmt=fmt, compact=True, **kw_p),
                exp_multi]
    caps = [cn.cloud_points(SW, SH, s), lib.fovea_multi_cloud_points(W, H, LEVELS[F], F, OFFSETS, s), lib.fovea_cloud_points(W, H, LEVELS[F], F, OFFSETS[0], s),
            cn.cloud_points(fw, fh, s), cn.cloud_points(W, H, s), lib.resized_cloud_points(W, H, FACTOR)]
    caps.append(caps[1])
    assert all(0 < e.size < cap for e, cap in zip(expected, caps))    # (every filter drops something and keeps something)

    with lib.Context(levels=LEVELS[F], fovea_levels=F, slots=1) as c:
        so, h = c.lib, c.handle
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        d_small, d_planes = [c.to_device(a) for a in small], [c.to_device(a) for a in planes]
        d_pts = [_poisoned(c, (cap + EXTRA) * item) for cap in caps]
        d_cnt = [c.to_device(np.full(1, -7, np.int64)) for _ in caps]
        d_per = {k: c.to_device(np.full(m + 1, -7, np.int64)) for k, m in ((1, E), (2, F), (6, E))}
        prm_f, prm_s, prm_p = (lib.cloud_params(sampling=s, format=fmt, compact=True, **kw) for kw in (kw_f, kw_s, kw_p))
        prm_r = lib.cloud_params(format=fmt, compact=True, **kw_p)
        sx, sy, sc = d_stacks[0], d_stacks[0] + 4 * F * fw * fh, d_stacks[0] + 8 * F * fw * fh
        ox, oy = c._offsets(OFFSETS, n)

        def multi(k):
            return so.ugsm_point_cloud_fovea_multi(h, 0, n, c._ptrs(d_stacks), W, H, ox, oy, d_rgb, 3 * W, *pp, C.byref(prm_f), d_pts[k], caps[k],
                                                   d_cnt[k], d_per[k])
        try:
            before = so.ugsm_context_device_bytes(h)
            c.check(so.ugsm_point_cloud(h, 0, d_small[0], d_small[1], d_small[2], d_small[3], SW, SH, 3 * SW, *pp, C.byref(prm_s), d_pts[0], caps[0],
                                        d_cnt[0]))
            grown = so.ugsm_context_device_bytes(h) - before
            c.check(multi(1))
            assert so.ugsm_context_device_bytes(h) - before > grown > 0    # (the count buffer: a few words, then regrown for E grids)
            c.check(so.ugsm_point_cloud_fovea_all(h, 0, sx, sy, sc, W, H, OFFSETS[0][0], OFFSETS[0][1], d_rgb, 3 * W, *pp, C.byref(prm_f), d_pts[2],
                                                  caps[2], d_cnt[2], d_per[2]))
            c.check(so.ugsm_point_cloud_fovea(h, 0, sx, sy, sc, fw, fh, 1, int(mapping[0]), int(mapping[1]), C.c_float(float(mapping[2])), d_rgb, W, H, 3 * W,
                                              *pp, C.byref(prm_f), d_pts[3], caps[3], d_cnt[3]))
            c.check(so.ugsm_point_cloud(h, 0, d_planes[0], d_planes[1], d_planes[2], d_planes[3], W, H, 3 * W, *pp, C.byref(prm_p), d_pts[4], caps[4],
                                        d_cnt[4]))
            c.check(so.ugsm_point_cloud_resized(h, 0, d_planes[0], d_planes[1], d_planes[2], d_planes[3], W, H, 3 * W, *pp, C.c_float(FACTOR),
                                                C.byref(prm_r), d_pts[5], caps[5], d_cnt[5]))
            c.check(multi(6))
            c.check(so.ugsm_wait(h, 0))

            names = ["33 x 7", "two windows", "window 0's stack", "its level 1", "320 x 240 planes", "resized by 0.3", "two windows again"]
            got = []
            for k, (name, exp, cap) in enumerate(zip(names, expected, caps)):
                count = int(c.to_host(d_cnt[k], (1,), np.int64)[0])
                print(f"s={s} fmt={fmt} {name}: count {count} of {cap} dense, expected {exp.size}")
                assert count == exp.size, name
                got.append(_read(c, lib, d_pts[k], cap, EXTRA, fmt, count))
                cn.assert_cloud_equal(got[k], exp, f"s={s} fmt={fmt} {name}")
            for k, per in ((1, per_multi), (2, per_stack), (6, per_multi)):
                words = c.to_host(d_per[k], (len(per) + 1,), np.int64).tolist()
                assert words == per + [-7], names[k]    # (the level / entry counts, and the word behind them untouched)
            assert got[6].tobytes() == got[1].tobytes()
        finally:
            for p in d_stacks + [d_rgb] + d_small + d_planes + d_pts + d_cnt + list(d_per.values()):
                c.free(p)
