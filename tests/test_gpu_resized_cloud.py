"""The resized cloud on the device (ugsm_point_cloud_resized / ugsm_point_cloud_resized_fovea) against the CPU restatement
(tests/resize_np.py): byte for byte, a NaN X, Y or Z equal to any NaN; and, independent of the restatement, against the dense cloud at
factor 1."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import resize_np as rn
from test_cloud_host import bad_argument_cases
from test_gpu_cloud import P1, P2, P2A, POISON, _inputs, _read
from test_resized_cloud_host import resized_bad_argument_cases

pytestmark = pytest.mark.gpu

FACTORS = (0.2, 0.3, 1 / 3, 0.5, 0.7, 1.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(levels=14, slots=2)
    yield c
    c.close()


def _resized(ctx, lib, dptr, W, H, P2_, factor, fmt=cn.PCL32, compact=False, cap=None, extra=64, **kw):
    d_dx, d_dy, d_conf, d_rgb = dptr
    params = lib.cloud_params(format=fmt, compact=compact, **kw)
    n_all = lib.resized_cloud_points(W, H, factor)
    cap = n_all if cap is None else cap
    d_pts = ctx.to_device(np.full((cap + extra) * cn.DTYPES[fmt].itemsize, POISON, np.uint8))
    d_cnt = ctx.to_device(np.full(1, -7, np.int64))
    try:
        n = ctx.point_cloud_resized(d_dx, d_dy, d_conf, d_rgb, W, H, 3 * W, P1, P2_, factor, params, d_pts, cap, d_cnt)
        return n, _read(ctx, lib, d_pts, cap, extra, fmt, n)
    finally:
        ctx.free(d_pts)
        ctx.free(d_cnt)


@pytest.mark.parametrize("W,H", [(7, 5), (3, 3), (41, 29), (317, 203), (1000, 31)])
def test_resized_cloud_matches_restatement_at_odd_sizes(lib, ctx, orc, W, H):
    """Factors 0.2, 0.3, 1/3, 0.5, 0.7, 1 (where both sides stay at least 1) x both formats x dense / compact (a Z window and
    min_conf), with NaN and +-inf in dx and conf."""
    rng = np.random.Generator(np.random.PCG64(W * 7919 + H))
    dx, dy, conf, rgb = _inputs(rng, W, H)
    P2_ = P2A if W != 1000 else P2
    dptr = [ctx.to_device(a) for a in (dx, dy, conf, rgb)]
    z = orc.triangulate(dx, dy, P1, P2_)[2]
    zf = z[np.isfinite(z)]
    zlo, zhi = (float(np.percentile(zf, q)) for q in (10, 90))
    try:
        ran = 0
        for f in FACTORS:
            if min(rn.resized_size(W, H, f)) < 1:
                assert lib.resized_cloud_points(W, H, f) == -1
                continue
            for fmt in (cn.PCL32, cn.XYZRGB16):
                for compact in (False, True):
                    kw = dict(min_conf=0.3, z_min=zlo, z_max=zhi) if compact else {}
                    n, got = _resized(ctx, lib, dptr, W, H, P2_, f, fmt, compact, **kw)
                    exp = rn.resized_cloud(orc, dx, dy, rgb, P1, P2_, f, conf=conf, fmt=fmt, compact=compact, **kw)
                    assert n == exp.size
                    cn.assert_cloud_equal(got, exp, f"{W}x{H} f={f:.4f} fmt={fmt} compact={compact}")
                    ran += 1
        assert ran >= 8
        if (W, H) == (7, 5):
            assert lib.resized_cloud_points(W, H, 0.2) == 1
    finally:
        for p in dptr:
            ctx.free(p)


def test_factor_one_equals_the_dense_cloud(lib, ctx):
    """Independent of the restatement: at factor 1 the resized cloud is ugsm_point_cloud's, byte for byte -- on planes whose Z is
    finite everywhere and (cv::resize copies an unchanged size) on salted ones; dense and compact, both formats."""
    rng = np.random.Generator(np.random.PCG64(11))
    W, H = 317, 203
    salted = _inputs(rng, W, H)
    clean = (rng.normal(-40, 5, (H, W)).astype(np.float32), rng.normal(0, 1, (H, W)).astype(np.float32), salted[2], salted[3])
    n_all = W * H
    d_a, d_b = ctx.alloc(n_all * 32), ctx.alloc(n_all * 32)
    d_cnt = ctx.alloc(8)
    try:
        for planes in (clean, salted):
            dptr = [ctx.to_device(a) for a in planes]
            try:
                for fmt in (cn.PCL32, cn.XYZRGB16):
                    for compact, kw in ((False, {}), (True, dict(min_conf=0.3))):
                        prm = lib.cloud_params(format=fmt, compact=compact, **kw)
                        n1 = ctx.point_cloud(*dptr, W, H, 3 * W, P1, P2A, prm, d_a, n_all, d_cnt)
                        n2 = ctx.point_cloud_resized(*dptr, W, H, 3 * W, P1, P2A, 1.0, prm, d_b, n_all, d_cnt)
                        assert n1 == n2 and n1 > 0
                        item = cn.DTYPES[fmt].itemsize
                        assert np.array_equal(ctx.to_host(d_a, (n1 * item,), np.uint8), ctx.to_host(d_b, (n2 * item,), np.uint8))
            finally:
                for p in dptr:
                    ctx.free(p)
    finally:
        for p in (d_a, d_b, d_cnt):
            ctx.free(p)


def test_cap_below_count_writes_exactly_cap_records(lib, ctx, orc):
    rng = np.random.Generator(np.random.PCG64(6))
    W, H = 317, 203
    dx, dy, conf, rgb = _inputs(rng, W, H)
    dptr = [ctx.to_device(a) for a in (dx, dy, conf, rgb)]
    try:
        for f in (0.2, 0.7):
            for fmt in (cn.PCL32, cn.XYZRGB16):
                for compact, kw in ((False, {}), (True, dict(min_conf=0.5))):
                    exp = rn.resized_cloud(orc, dx, dy, rgb, P1, P2A, f, conf=conf, fmt=fmt, compact=compact, **kw)
                    for cap in (0, 1, 65, exp.size // 2 + 3, exp.size - 1):
                        n, got = _resized(ctx, lib, dptr, W, H, P2A, f, fmt, compact, cap=cap, extra=100, **kw)
                        assert n == exp.size and got.size == cap
                        cn.assert_cloud_equal(got, exp[:cap], f"f={f} cap {cap} fmt={fmt} compact={compact}")
    finally:
        for p in dptr:
            ctx.free(p)


def test_16mp_after_submit_full_on_the_same_slot(lib, orc, oracle_16mp):
    """ugsm_submit_full on the 16 MP pair, then the resized cloud on the same slot with no wait in between, against the restatement of
    the oracle's field: 985 x 652 points at f = 0.2 (dense PCL32, compact PCL32), and f = 0.5 dense 16-byte."""
    g = oracle_16mp
    W, H, L, R, full = g["W"], g["H"], g["L"], g["R"], g["full"]
    c = lib.Context(levels=14, slots=2)
    try:
        pL, pR = c.to_device(L), c.to_device(R)
        d_out = c.alloc(3 * W * H * 4)
        plane = W * H * 4
        cap = lib.resized_cloud_points(W, H, 0.5)
        d_pts, d_cnt = c.alloc(cap * 32), c.alloc(8)
        c.check(c.lib.ugsm_submit_full(c.handle, 1, pL, pR, W, H, L.strides[0], d_out))
        n = c.point_cloud_resized(d_out, d_out + plane, d_out + 2 * plane, pL, W, H, L.strides[0], P1, P2, 0.2, lib.cloud_params(), d_pts,
                                  cap, d_cnt, slot=1)
        assert n == 985 * 652
        cn.assert_cloud_equal(c.cloud_to_host(d_pts, n), rn.resized_cloud(orc, full[0], full[1], L, P1, P2, 0.2),
                              "16 MP f=0.2 dense PCL32 after submit_full")
        z = orc.triangulate(full[0], full[1], P1, P2)[2]
        zf = z[np.isfinite(z)]
        kw = dict(min_conf=0.25, z_min=float(np.percentile(zf, 5)), z_max=float(np.percentile(zf, 95)))
        exp = rn.resized_cloud(orc, full[0], full[1], L, P1, P2, 0.2, conf=full[2], compact=True, **kw)
        assert 0 < exp.size < 985 * 652
        n = c.point_cloud_resized(d_out, d_out + plane, d_out + 2 * plane, pL, W, H, L.strides[0], P1, P2, 0.2,
                                  lib.cloud_params(compact=True, **kw), d_pts, cap, d_cnt, slot=1)
        assert n == exp.size
        cn.assert_cloud_equal(c.cloud_to_host(d_pts, n), exp, "16 MP f=0.2 compact PCL32")
        n = c.point_cloud_resized(d_out, d_out + plane, d_out + 2 * plane, pL, W, H, L.strides[0], P1, P2, 0.5,
                                  lib.cloud_params(format=lib.UGSM_CLOUD_XYZRGB16), d_pts, cap, d_cnt, slot=0)
        cn.assert_cloud_equal(c.cloud_to_host(d_pts, n, lib.UGSM_CLOUD_XYZRGB16),
                              rn.resized_cloud(orc, full[0], full[1], L, P1, P2, 0.5, fmt=cn.XYZRGB16), "16 MP f=0.5 dense 16-byte")
        for p in (pL, pR, d_out, d_pts, d_cnt):
            c.free(p)
    finally:
        c.close()


def test_foveated_resized_cloud_on_the_16mp_stack(lib, ctx, orc, oracle_16mp):
    """ugsm_point_cloud_resized_fovea at src_level 0, 3 and 6 of the oracle's 16 MP fovea stack with ugsm_fovea_mapping's margins, the
    colour unmapped (the reference's) and mapped, dense and compact; and at factor 1 with the mapped colour it is
    ugsm_point_cloud_fovea's cloud byte for byte."""
    g = oracle_16mp
    W, H, L, stack = g["W"], g["H"], g["L"], g["stack"]
    _, F, fh, fw = stack.shape
    sx, sy, sc = (np.ascontiguousarray(stack[k]) for k in range(3))
    dptr = [ctx.to_device(a) for a in (sx, sy, sc, L)]
    n_all = fw * fh
    d_pts, d_ref = ctx.alloc(n_all * 32 + 4096), ctx.alloc(n_all * 32 + 4096)
    d_cnt = ctx.alloc(8)
    try:
        for src in (0, 3, 6):
            left, upper, scale = lib.fovea_mapping(W, H, src)
            for mapped in (0, 1):
                for f, fmt, compact, kw in ((0.2, cn.PCL32, False, {}), (0.2, cn.XYZRGB16, True, dict(min_conf=0.2)),
                                            (0.5, cn.PCL32, True, dict(min_conf=0.1))):
                    exp = rn.resized_cloud_fovea(orc, sx, sy, src, left, upper, scale, L, P1, P2, f, stackc=sc, colour_mapped=mapped,
                                                 fmt=fmt, compact=compact, **kw)
                    n = ctx.point_cloud_resized_fovea(dptr[0], dptr[1], dptr[2], fw, fh, src, left, upper, scale, dptr[3], W, H,
                                                      L.strides[0], P1, P2, f, lib.cloud_params(format=fmt, compact=compact, **kw), d_pts,
                                                      n_all, d_cnt, colour_mapped=mapped)
                    assert n == exp.size
                    cn.assert_cloud_equal(ctx.cloud_to_host(d_pts, n, fmt), exp,
                                          f"fovea level {src} f={f} mapped={mapped} fmt={fmt} compact={compact}")
            prm = lib.cloud_params(compact=True, min_conf=0.2)
            n1 = ctx.point_cloud_fovea(dptr[0], dptr[1], dptr[2], fw, fh, src, left, upper, scale, dptr[3], W, H, L.strides[0], P1, P2,
                                       prm, d_ref, n_all, d_cnt)
            n2 = ctx.point_cloud_resized_fovea(dptr[0], dptr[1], dptr[2], fw, fh, src, left, upper, scale, dptr[3], W, H, L.strides[0],
                                               P1, P2, 1.0, prm, d_pts, n_all, d_cnt, colour_mapped=1)
            assert n1 == n2 > 0
            assert np.array_equal(ctx.to_host(d_ref, (n1 * 32,), np.uint8), ctx.to_host(d_pts, (n2 * 32,), np.uint8)), f"level {src}"
    finally:
        for p in dptr + [d_pts, d_ref, d_cnt]:
            ctx.free(p)


def test_bad_arguments_on_a_live_context_write_nothing(lib, ctx):
    """Every refusal of the cloud and of the resized forms, on a live context with real buffers: UGSM_ERR_BAD_ARG, and neither the
    points nor the count touched; then calls that pass."""
    W, H = 64, 32
    bufs = dict(dx=ctx.alloc(W * H * 4), dy=ctx.alloc(W * H * 4), conf=ctx.alloc(W * H * 4), rgb=ctx.alloc(3 * W * H),
                points=ctx.to_device(np.full(8192, POISON, np.uint8)), count=ctx.to_device(np.full(1, -7, np.int64)))
    so = lib.load()
    P = (C.c_double * 12)(*P1.reshape(12))

    def call(fovea, factor=0.2, colour_mapped=0, **over):
        a = dict(bufs, W=W, H=H, stride=3 * W, P1=P, P2=P, p=lib.cloud_params(), cap=100)
        if "points" in over and over["points"] is not None and over["points"] < 0x100000:
            over["points"] = bufs["points"] + 8       # (the misaligned case)
        a.update(over)
        p = C.byref(a["p"]) if a["p"] is not None else None
        if fovea:
            return so.ugsm_point_cloud_resized_fovea(ctx.handle, 0, a["dx"], a["dy"], a["conf"], 40, 20, 0, 8, 6, C.c_float(1.0), a["rgb"],
                                                     a["W"], a["H"], a["stride"], a["P1"], a["P2"], C.c_float(factor), colour_mapped, p,
                                                     a["points"], a["cap"], a["count"])
        return so.ugsm_point_cloud_resized(ctx.handle, 0, a["dx"], a["dy"], a["conf"], a["rgb"], a["W"], a["H"], a["stride"], a["P1"],
                                           a["P2"], C.c_float(factor), p, a["points"], a["cap"], a["count"])

    def untouched():
        ctx.check(so.ugsm_wait(ctx.handle, 0))
        return (ctx.to_host(bufs["points"], (8192,), np.uint8) == POISON).all() and ctx.to_host(bufs["count"], (1,), np.int64)[0] == -7
    try:
        for fovea in (False, True):
            for name, over in bad_argument_cases(lib) + resized_bad_argument_cases(lib):
                if name == "colour_mapped 2" and not fovea:
                    continue
                assert call(fovea, **dict(over)) == lib.UGSM_ERR_BAD_ARG, (name, fovea)
        assert so.ugsm_point_cloud_resized(ctx.handle, 5, bufs["dx"], bufs["dy"], None, bufs["rgb"], W, H, 3 * W, P, P, C.c_float(0.5),
                                           C.byref(lib.cloud_params()), bufs["points"], 100, bufs["count"]) == lib.UGSM_ERR_BAD_ARG
        assert untouched()
        assert call(False) == lib.UGSM_OK
        ctx.check(so.ugsm_wait(ctx.handle, 0))
        assert ctx.to_host(bufs["count"], (1,), np.int64)[0] == lib.resized_cloud_points(W, H, 0.2) == 12 * 6
        assert call(True, colour_mapped=1) == lib.UGSM_OK
        ctx.check(so.ugsm_wait(ctx.handle, 0))
        assert ctx.to_host(bufs["count"], (1,), np.int64)[0] == lib.resized_cloud_points(40, 20, 0.2) == 8 * 4
    finally:
        for p in bufs.values():
            ctx.free(p)
