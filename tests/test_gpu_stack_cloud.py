"""The merged cloud of the whole fovea stack on the device (ugsm_point_cloud_fovea_all) against the CPU restatement
(tests/stack_cloud_np.py) and against the per-level call it generalises: byte for byte, a NaN X, Y or Z equal to any NaN."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import encode_np as en
import stack_cloud_np as sn
from test_gpu_cloud import P1, P2, P2A, POISON, _inputs, _poisoned, _read
from test_stack_cloud_host import bad_argument_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(levels=14, fovea_levels=7, slots=2)
    yield c
    c.close()


def _all(ctx, lib, dptr, W, H, off, stride, P2_, fmt, s, compact, cap=None, extra=64, slot=0, **kw):
    """One merged cloud into a poisoned buffer -> (count, the records written, the per-level counts); checks the bytes behind them."""
    d_sx, d_sy, d_sc, d_rgb = dptr
    F = ctx.cfg.fovea_levels
    params = lib.cloud_params(sampling=s, format=fmt, compact=compact, **kw)
    if cap is None:
        cap = lib.fovea_cloud_points(W, H, ctx.cfg.levels, F, off, s)
    d_pts = _poisoned(ctx, (cap + extra) * cn.DTYPES[fmt].itemsize)
    d_cnt = ctx.to_device(np.full(1, -7, np.int64))
    d_lvl = ctx.to_device(np.full(F, -7, np.int64))
    try:
        n, per = ctx.point_cloud_fovea_all(d_sx, d_sy, d_sc, W, H, off, d_rgb, stride, P1, P2_, params, d_pts, cap, d_cnt, d_lvl, slot=slot)
        return n, _read(ctx, lib, d_pts, cap, extra, fmt, n), per
    finally:
        for p in (d_pts, d_cnt, d_lvl):
            ctx.free(p)


def _per_level(c, lib, dptr, W, H, levels, F, off, fmt, s):
    """The dense cloud of every level from ugsm_point_cloud_fovea with ugsm_fovea_level_mapping's numbers: a list of record arrays."""
    fw, fh = sn.fovea_dims(W, H, F)
    d_pts, d_cnt = c.alloc(fw * fh * 32), c.alloc(8)
    out = []
    try:
        for k in range(F):
            left, upper, scale = lib.fovea_level_mapping(W, H, levels, F, k, off)
            n = c.point_cloud_fovea(dptr[0], dptr[1], dptr[2], fw, fh, k, left, upper, scale, dptr[3], W, H, 3 * W, P1, P2A,
                                    lib.cloud_params(sampling=s, format=fmt), d_pts, fw * fh, d_cnt)
            assert n == cn.cloud_points(fw, fh, s)
            out.append(c.cloud_to_host(d_pts, n, fmt))
    finally:
        c.free(d_pts)
        c.free(d_cnt)
    return out


def _random_stack(rng, W, H, F):
    fw, fh = sn.fovea_dims(W, H, F)
    sx, sy, sc, _ = _inputs(rng, fw, F * fh)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return [a.reshape(F, fh, fw) for a in (sx, sy, sc)] + [rgb]


@pytest.mark.parametrize("W,H,levels,F,off", [(160, 120, 14, 7, (0, 0)), (160, 120, 14, 7, (23, -17)), (320, 240, 9, 4, (0, 0)),
                                              (320, 240, 9, 4, (-60, 40))])
def test_random_stacks_match_the_restatement(lib, orc, W, H, levels, F, off):
    """Both record formats x dense / compact x sampling 1 and 3 on stacks with NaN, inf and wild disparities: the count, the bytes and
    the per-level counts.  About 4 % of the pixels carry a NaN or +-inf disparity, whose integer conversion C leaves undefined (the
    oracle's x86 build and the device differ there: stack_cloud_np's note): their X, Y, Z are compared with ugsm_point_cloud_fovea's
    record for the pixel, everything else with the oracle."""
    rng = np.random.Generator(np.random.PCG64(W * 100 + F * 10 + off[0] % 7))
    sx, sy, sc, rgb = _random_stack(rng, W, H, F)
    with lib.Context(levels=levels, fovea_levels=F) as c:
        dptr = [c.to_device(a) for a in (sx, sy, sc, rgb)]
        zs = np.concatenate([orc.triangulate_fovea(sx, sy, k, *sn.level_mapping(W, H, F, k, off), P1, P2A)[2].reshape(-1) for k in range(F)])
        zlo, zhi = (float(np.percentile(zs[np.isfinite(zs)], q)) for q in (10, 90))
        assert 0 < sum(int(sn.undefined_conversion(sx, sy, k).sum()) for k in range(F)) < sx.size // 10
        for s in (1, 3):
            for fmt in (cn.PCL32, cn.XYZRGB16):
                und = _per_level(c, lib, dptr, W, H, levels, F, off, fmt, s)
                for compact in (False, True):
                    kw = dict(min_conf=0.3, z_min=zlo, z_max=zhi) if compact else {}
                    exp, exp_per = sn.cloud_fovea_all(orc, sx, sy, rgb, off, P1, P2A, stackc=sc, s=s, fmt=fmt, compact=compact, undefined=und,
                                                      **kw)
                    n, got, per = _all(c, lib, dptr, W, H, off, 3 * W, P2A, fmt, s, compact, **kw)
                    what = f"{W}x{H} F={F} off={off} s={s} fmt={fmt} compact={compact}"
                    assert n == exp.size and per == exp_per, what
                    if not compact:
                        assert (n, per) == lib.fovea_cloud_points(W, H, levels, F, off, s, per_level=True)
                    cn.assert_cloud_equal(got, exp, what)
        # a compact cloud without a confidence plane, and without the per-level counts
        exp, _ = sn.cloud_fovea_all(orc, sx, sy, rgb, off, P1, P2A, s=1, fmt=cn.XYZRGB16, compact=True,
                                    undefined=_per_level(c, lib, dptr, W, H, levels, F, off, cn.XYZRGB16, 1))
        d_pts, d_cnt = c.alloc(exp.size * 16 + 16), c.alloc(8)
        n = c.point_cloud_fovea_all(dptr[0], dptr[1], None, W, H, off, dptr[3], 3 * W, P1, P2A,
                                    lib.cloud_params(format=cn.XYZRGB16, compact=True), d_pts, exp.size, d_cnt)
        assert n == exp.size
        cn.assert_cloud_equal(c.cloud_to_host(d_pts, n, cn.XYZRGB16), exp, "compact, no confidence plane, no level counts")
        for p in dptr + [d_pts, d_cnt]:
            c.free(p)


def test_merged_cloud_is_the_per_level_clouds_without_the_covered_records(lib, orc):
    """ugsm_point_cloud_fovea per level with ugsm_fovea_level_mapping's numbers, the covered records dropped on the host: concatenated,
    that is the merged cloud byte for byte, dense, in both formats."""
    W, H, levels, F, off = 320, 240, 9, 4, (-60, 40)
    rng = np.random.Generator(np.random.PCG64(11))
    sx, sy, sc, rgb = _random_stack(rng, W, H, F)
    fw, fh = sn.fovea_dims(W, H, F)
    with lib.Context(levels=levels, fovea_levels=F) as c:
        dptr = [c.to_device(a) for a in (sx, sy, sc, rgb)]
        d_pts, d_cnt = c.alloc(fw * fh * 32), c.alloc(8)
        for s in (1, 2):
            for fmt in (cn.PCL32, cn.XYZRGB16):
                item = cn.DTYPES[fmt].itemsize
                parts = []
                for k in range(F):
                    left, upper, scale = lib.fovea_level_mapping(W, H, levels, F, k, off)
                    n = c.point_cloud_fovea(dptr[0], dptr[1], dptr[2], fw, fh, k, left, upper, scale, dptr[3], W, H, 3 * W, P1, P2A,
                                            lib.cloud_params(sampling=s, format=fmt), d_pts, fw * fh, d_cnt)
                    cols, rows = sn.covered(W, H, F, k, off)
                    keep = ~np.outer(cols[::s], rows[::s]).reshape(-1)
                    assert n == keep.size
                    parts.append(c.to_host(d_pts, (n, item), np.uint8)[keep])
                exp = np.concatenate(parts).reshape(-1)
                n, got, per = _all(c, lib, dptr, W, H, off, 3 * W, P2A, fmt, s, False)
                assert n * item == exp.size and per == [p.shape[0] for p in parts]
                assert np.array_equal(got.view(np.uint8), exp), f"s={s} fmt={fmt}"
        for p in dptr + [d_pts, d_cnt]:
            c.free(p)


def test_merged_cloud_of_the_16mp_stack(lib, ctx, orc, oracle_16mp):
    """The oracle's 16 MP stack: dense PCL32 (1 005 221 points), and compact 16-byte with min_conf 0.2 and a Z window (twice: the same
    bytes)."""
    g = oracle_16mp
    W, H, L, stack = g["W"], g["H"], g["L"], g["stack"]
    sx, sy, sc = (np.ascontiguousarray(stack[k]) for k in range(3))
    dptr = [ctx.to_device(a) for a in (sx, sy, sc, L)]
    try:
        exp, exp_per = sn.cloud_fovea_all(orc, sx, sy, L, (0, 0), P1, P2, stackc=sc)
        n, got, per = _all(ctx, lib, dptr, W, H, (0, 0), L.strides[0], P2, cn.PCL32, 1, False)
        assert n == 1005221 == exp.size and per == exp_per == lib.fovea_cloud_points(W, H, 14, 7, per_level=True)[1]
        cn.assert_cloud_equal(got, exp, "16 MP dense PCL32")
        zf = exp["z"][np.isfinite(exp["z"])]
        kw = dict(min_conf=0.2, z_min=float(np.percentile(zf, 5)), z_max=float(np.percentile(zf, 95)))
        exp, exp_per = sn.cloud_fovea_all(orc, sx, sy, L, (0, 0), P1, P2, stackc=sc, fmt=cn.XYZRGB16, compact=True, **kw)
        assert 0 < exp.size < n
        raw = []
        for _ in range(2):
            nc, got, per = _all(ctx, lib, dptr, W, H, (0, 0), L.strides[0], P2, cn.XYZRGB16, 1, True, cap=n, **kw)
            assert nc == exp.size and per == exp_per
            raw.append(got.tobytes())
        assert raw[0] == raw[1], "two compact runs differ"
        cn.assert_cloud_equal(got, exp, "16 MP compact 16-byte")
    finally:
        for p in dptr:
            ctx.free(p)


def test_cap_below_count_writes_exactly_cap_records(lib, orc):
    W, H, levels, F, off = 320, 240, 9, 4, (0, 0)
    rng = np.random.Generator(np.random.PCG64(5))
    sx, sy, sc, rgb = _random_stack(rng, W, H, F)
    with lib.Context(levels=levels, fovea_levels=F) as c:
        dptr = [c.to_device(a) for a in (sx, sy, sc, rgb)]
        for fmt in (cn.PCL32, cn.XYZRGB16):
            und = _per_level(c, lib, dptr, W, H, levels, F, off, fmt, 1)
            for compact, kw in ((False, {}), (True, dict(min_conf=0.5))):
                exp, exp_per = sn.cloud_fovea_all(orc, sx, sy, rgb, off, P1, P2A, stackc=sc, fmt=fmt, compact=compact, undefined=und, **kw)
                for cap in (0, 1, 97, exp_per[0] + 5, exp.size // 2 + 3, exp.size - 1):
                    n, got, per = _all(c, lib, dptr, W, H, off, 3 * W, P2A, fmt, 1, compact, cap=cap, extra=100, **kw)
                    assert n == exp.size and got.size == cap and per == exp_per   # (the counts are the cloud's, not what was written)
                    cn.assert_cloud_equal(got, exp[:cap], f"cap {cap} fmt={fmt} compact={compact}")
        for p in dptr:
            c.free(p)


def test_compact_cloud_is_deterministic(lib, orc):
    W, H, levels, F, off = 320, 240, 9, 4, (17, 9)
    rng = np.random.Generator(np.random.PCG64(6))
    sx, sy, sc, rgb = _random_stack(rng, W, H, F)
    with lib.Context(levels=levels, fovea_levels=F) as c:
        dptr = [c.to_device(a) for a in (sx, sy, sc, rgb)]
        runs = [_all(c, lib, dptr, W, H, off, 3 * W, P2A, cn.PCL32, 1, True, min_conf=0.4) for _ in range(3)]
        assert runs[0][0] > 0
        for n, got, per in runs[1:]:
            assert n == runs[0][0] and per == runs[0][2] and got.tobytes() == runs[0][1].tobytes()
        for p in dptr:
            c.free(p)


def test_end_to_end_after_submit_foveated_on_the_same_slot(lib, ctx, orc):
    """ugsm_submit_foveated at 1280 x 960 with a window offset, then the merged cloud on the same slot with no wait in between (stream
    order), against the restatement on the oracle's stack."""
    from ug_stereomatcher_amd import synth
    W, H, off = 1280, 960, (90, -40)
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 31)
    stack = orc.match_foveated(L, R, 14, 7, off[0], off[1])[0]
    _, F, fh, fw = stack.shape
    exp, exp_per = sn.cloud_fovea_all(orc, stack[0], stack[1], L, off, P1, P2, stackc=stack[2], compact=True, min_conf=0.2)
    dense, dense_per = sn.cloud_fovea_all(orc, stack[0], stack[1], L, off, P1, P2)
    pL, pR = ctx.to_device(L), ctx.to_device(R)
    lvl = F * fh * fw * 4
    d_stack = ctx.alloc(3 * lvl)
    d_pts, d_cnt, d_lvl = ctx.alloc(dense.size * 32), ctx.alloc(8), ctx.alloc(8 * F)
    try:
        for params, want, want_per in ((lib.cloud_params(compact=True, min_conf=0.2), exp, exp_per), (lib.cloud_params(), dense, dense_per)):
            ctx.check(ctx.lib.ugsm_submit_foveated(ctx.handle, 1, pL, pR, W, H, L.strides[0], off[0], off[1], d_stack, None, None))
            n, per = ctx.point_cloud_fovea_all(d_stack, d_stack + lvl, d_stack + 2 * lvl, W, H, off, pL, L.strides[0], P1, P2, params, d_pts,
                                               dense.size, d_cnt, d_lvl, slot=1)
            assert n == want.size and per == want_per
            cn.assert_cloud_equal(ctx.cloud_to_host(d_pts, n), want, f"1280 x 960 after submit_foveated, compact={params.compact}")
    finally:
        for p in (pL, pR, d_stack, d_pts, d_cnt, d_lvl):
            ctx.free(p)


def test_bgra8_image_gives_the_cloud_of_its_rgb8_conversion(lib, orc):
    W, H, levels, F, off = 320, 240, 9, 4, (0, 0)
    rng = np.random.Generator(np.random.PCG64(8))
    sx, sy, sc, rgb = _random_stack(rng, W, H, F)
    img = en.encode(rgb, en.BGRA8)
    assert np.array_equal(en.to_rgb8(img, en.BGRA8), rgb)
    with lib.Context(levels=levels, fovea_levels=F) as c:
        dptr = [c.to_device(a) for a in (sx, sy, sc, rgb)]
        d_img = c.to_device(img)
        n0, rec0, per0 = _all(c, lib, dptr, W, H, off, 3 * W, P2A, cn.PCL32, 1, False)
        c.set_input_format(en.BGRA8)
        n1, rec1, per1 = _all(c, lib, dptr[:3] + [d_img], W, H, off, 4 * W, P2A, cn.PCL32, 1, False)
        # (the stride is checked against this format's four bytes per pixel; refused before anything is touched)
        assert c.lib.ugsm_point_cloud_fovea_all(c.handle, 0, dptr[0], dptr[1], dptr[2], W, H, 0, 0, d_img, 4 * W - 1, *_p12(),
                                                C.byref(lib.cloud_params()), dptr[0], 0, dptr[1], None) == lib.UGSM_ERR_BAD_ARG
        c.set_input_format(en.RGB8)
        assert (n0, per0) == (n1, per1) and rec0.tobytes() == rec1.tobytes()
        und = _per_level(c, lib, dptr, W, H, levels, F, off, cn.PCL32, 1)
        cn.assert_cloud_equal(rec1, sn.cloud_fovea_all(orc, sx, sy, rgb, off, P1, P2A, undefined=und)[0], "bgra8")
        for p in dptr + [d_img]:
            c.free(p)


def _p12():
    P = (C.c_double * 12)(*P1.reshape(12))
    return P, P


def test_bad_arguments_on_a_live_context(lib):
    """Every refusal of the host test on a live context with real buffers (large enough that nothing could be touched out of bounds
    even if a check were missing), a context whose stack has one level, a slot that does not exist; then a call that passes."""
    W, H, levels, F = 320, 240, 9, 4
    fw, fh = sn.fovea_dims(W, H, F)
    P = _p12()[0]
    with lib.Context(levels=levels, fovea_levels=F) as c:
        plane = F * fw * fh * 4
        bufs = dict(dx=c.to_device(np.zeros(plane, np.uint8)), dy=c.to_device(np.zeros(plane, np.uint8)),
                    conf=c.to_device(np.zeros(plane, np.uint8)), rgb=c.to_device(np.zeros(3 * W * H, np.uint8)),
                    points=c.alloc(F * fw * fh * 32), count=c.alloc(8), level_counts=c.alloc(8 * F))
        so = lib.load()

        def call(handle=c.handle, slot=0, **over):
            a = dict(bufs, W=W, H=H, stride=3 * W, P1=P, P2=P, p=lib.cloud_params(), cap=100)
            if over.get("points") is not None:
                over["points"] = bufs["points"] + 8            # (the misaligned cases, at real addresses)
            if over.get("level_counts") is not None:
                over["level_counts"] = bufs["level_counts"] + 4
            if over.get("stride") == 191:
                over["stride"] = 3 * W - 1                     # (one byte short of this image's rows)
            a.update(over)
            p = C.byref(a["p"]) if a["p"] is not None else None
            return so.ugsm_point_cloud_fovea_all(handle, slot, a["dx"], a["dy"], a["conf"], a["W"], a["H"], 0, 0, a["rgb"], a["stride"], a["P1"],
                                                 a["P2"], p, a["points"], a["cap"], a["count"], a["level_counts"])
        try:
            for name, over in bad_argument_cases(lib):
                assert call(**dict(over)) == lib.UGSM_ERR_BAD_ARG, name
            assert call(slot=5) == lib.UGSM_ERR_BAD_ARG                       # (no such slot)
            assert call(W=2, H=2, stride=6) != lib.UGSM_OK                    # (too small for the stack's four levels)
            with lib.Context(levels=8, fovea_levels=1) as one:                # a one-level stack is the full frame: ugsm_point_cloud
                assert call(handle=one.handle) == lib.UGSM_ERR_BAD_ARG
            c.check(so.ugsm_wait(c.handle, 0))
            assert call() == lib.UGSM_OK and call(level_counts=None) == lib.UGSM_OK
            c.check(so.ugsm_wait(c.handle, 0))
        finally:
            for p in bufs.values():
                c.free(p)
