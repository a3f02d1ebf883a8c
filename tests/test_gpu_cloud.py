"""The coloured point cloud on the device (ugsm_point_cloud / ugsm_point_cloud_fovea) against the CPU restatement (tests/cloud_np.py):
byte for byte, a NaN X, Y or Z equal to any NaN."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
from test_cloud_host import bad_argument_cases

pytestmark = pytest.mark.gpu

P1 = np.array([[7.3230899280915291e+03, 0., 2.4836974544986647e+03, 0.],
               [0., 7.3035803715514758e+03, 1.7170248033347561e+03, 0.], [0., 0., 1., 0.]])
P2A = np.array([[6.78780819e+03, -1.92174329e+02, 3.52550369e+03, -2.01574768e+03],
                [2.8e+02, 7.29e+03, 1.69e+03, 3.1e+01], [2.0e-01, 1.0e-02, 9.8e-01, 3.0e-03]])
P2 = P1.copy()          # the 16 MP rig: rectified, 0.12 baseline (test_gpu_parity.py)
P2[0, 3] = -7.3230899280915291e+03 * 0.12
POISON = 0xA5


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


def _poisoned(ctx, nbytes):
    return ctx.to_device(np.full(nbytes, POISON, np.uint8))


def _read(ctx, lib, d_points, cap, extra, fmt, count):
    """The records written (min(count, cap)) and a check that the `extra` records of poison behind them are intact."""
    item = cn.DTYPES[fmt].itemsize
    raw = ctx.to_host(d_points, ((cap + extra) * item,), np.uint8)
    n = min(count, cap)
    assert (raw[n * item:] == POISON).all(), "a byte past the records written was touched"
    return raw[:n * item].view(cn.DTYPES[fmt])


def _cloud(ctx, lib, dptr, W, H, stride, P2_, fmt, s, compact, cap=None, extra=64, min_conf=None, z_min=None, z_max=None):
    d_dx, d_dy, d_conf, d_rgb = dptr
    params = lib.cloud_params(sampling=s, format=fmt, compact=compact, min_conf=min_conf, z_min=z_min, z_max=z_max)
    cap = cn.cloud_points(W, H, s) if cap is None else cap
    d_pts = _poisoned(ctx, (cap + extra) * cn.DTYPES[fmt].itemsize)
    d_cnt = ctx.to_device(np.full(1, -7, np.int64))
    try:
        n = ctx.point_cloud(d_dx, d_dy, d_conf, d_rgb, W, H, stride, P1, P2_, params, d_pts, cap, d_cnt)
        return n, _read(ctx, lib, d_pts, cap, extra, fmt, n)
    finally:
        ctx.free(d_pts)
        ctx.free(d_cnt)


def _inputs(rng, W, H):
    dx = rng.normal(-40, 25, (H, W)).astype(np.float32)
    dy = rng.normal(0, 2, (H, W)).astype(np.float32)
    conf = rng.uniform(0, 1, (H, W)).astype(np.float32)
    for a, vals in ((dx, (np.nan, np.inf, -np.inf)), (conf, (np.nan, np.inf, -np.inf))):
        for v in vals:
            a.flat[rng.integers(0, a.size, max(1, a.size // 50))] = v
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return dx, dy, conf, rgb


@pytest.mark.parametrize("W,H", [(33, 7), (317, 203), (1000, 31)])
def test_cloud_matches_restatement_at_odd_sizes(lib, ctx, orc, W, H):
    """Both formats x dense / compact x sampling 1, 2, 3, 7, with NaN and +-inf in dx and conf; the compact form filters on the
    confidence and a Z window."""
    rng = np.random.Generator(np.random.PCG64(W * 1000 + H))
    dx, dy, conf, rgb = _inputs(rng, W, H)
    P2_ = P2A if W != 1000 else P2
    dptr = [ctx.to_device(a) for a in (dx, dy, conf, rgb)]
    xyz = orc.triangulate(dx, dy, P1, P2_)
    word = cn.colour_word(rgb)
    zlo, zhi = (float(np.nanpercentile(xyz[2][np.isfinite(xyz[2])], q)) for q in (10, 90))
    try:
        before = lib.load().ugsm_context_device_bytes(ctx.handle)
        for s in (1, 2, 3, 7):
            for fmt in (cn.PCL32, cn.XYZRGB16):
                for compact in (False, True):
                    kw = dict(min_conf=0.3, z_min=zlo, z_max=zhi) if compact else {}
                    n, got = _cloud(ctx, lib, dptr, W, H, 3 * W, P2_, fmt, s, compact, **kw)
                    exp = cn.records(xyz, word, s=s, fmt=fmt, conf=conf, compact=compact, **kw)
                    assert n == exp.size
                    cn.assert_cloud_equal(got, exp, f"{W}x{H} s={s} fmt={fmt} compact={compact}")
        after = lib.load().ugsm_context_device_bytes(ctx.handle)
        assert after > 0 and after >= before   # (the compact form's count buffer is the context's)
        # a compact cloud with the confidence plane but no confidence threshold drops only the NaN confidences (and non-finite points)
        n, got = _cloud(ctx, lib, dptr, W, H, 3 * W, P2_, cn.XYZRGB16, 1, True)
        cn.assert_cloud_equal(got, cn.records(xyz, word, conf=conf, compact=True, fmt=cn.XYZRGB16), f"{W}x{H} compact, no threshold")
        # ... and without a plane there is no confidence test
        n, got = _cloud(ctx, lib, [dptr[0], dptr[1], None, dptr[3]], W, H, 3 * W, P2_, cn.XYZRGB16, 2, True)
        cn.assert_cloud_equal(got, cn.records(xyz, word, s=2, compact=True, fmt=cn.XYZRGB16), f"{W}x{H} compact, no confidence plane")
    finally:
        for p in dptr:
            ctx.free(p)


def test_cloud_with_row_padding_like_cv_mat_step(lib, ctx, orc):
    rng = np.random.Generator(np.random.PCG64(77))
    W, H, stride = 317, 203, 3 * 317 + 13
    dx, dy, conf, rgb = _inputs(rng, W, H)
    padded = np.zeros((H, stride), np.uint8)
    padded[:, :3 * W] = rgb.reshape(H, 3 * W)
    dptr = [ctx.to_device(a) for a in (dx, dy, conf, padded)]
    try:
        n, got = _cloud(ctx, lib, dptr, W, H, stride, P2A, cn.PCL32, 1, False)
        cn.assert_cloud_equal(got, cn.cloud(orc, dx, dy, rgb, P1, P2A), "strided rgb rows")
    finally:
        for p in dptr:
            ctx.free(p)


def test_cap_below_count_writes_exactly_cap_records(lib, ctx, orc):
    rng = np.random.Generator(np.random.PCG64(5))
    W, H = 317, 203
    dx, dy, conf, rgb = _inputs(rng, W, H)
    dptr = [ctx.to_device(a) for a in (dx, dy, conf, rgb)]
    xyz, word = orc.triangulate(dx, dy, P1, P2A), cn.colour_word(rgb)
    try:
        for fmt in (cn.PCL32, cn.XYZRGB16):
            for compact, kw in ((False, {}), (True, dict(min_conf=0.5))):
                exp = cn.records(xyz, word, fmt=fmt, conf=conf, compact=compact, **kw)
                for cap in (0, 1, 97, exp.size // 2 + 3, exp.size - 1):
                    n, got = _cloud(ctx, lib, dptr, W, H, 3 * W, P2A, fmt, 1, compact, cap=cap, extra=100, **kw)
                    assert n == exp.size and got.size == cap
                    cn.assert_cloud_equal(got, exp[:cap], f"cap {cap} fmt={fmt} compact={compact}")
    finally:
        for p in dptr:
            ctx.free(p)


def test_16mp_end_to_end_after_submit_full_on_the_same_slot(lib, orc, oracle_16mp):
    """ugsm_submit_full on the 16 MP pair, then ugsm_point_cloud on the same slot with no wait in between (stream order), against the
    restatement of the oracle's field: dense PCL32, then compact (twice: identical bytes) and dense 16-byte at sampling 2."""
    g = oracle_16mp
    W, H, L, R, full = g["W"], g["H"], g["L"], g["R"], g["full"]
    xyz, word = orc.triangulate(full[0], full[1], P1, P2), cn.colour_word(L)
    c = lib.Context(levels=14, slots=2)
    try:
        pL, pR = c.to_device(L), c.to_device(R)
        d_out = c.alloc(3 * W * H * 4)
        n_all = W * H
        d_pts = c.alloc(n_all * 32)
        d_cnt = c.alloc(8)
        plane = W * H * 4
        c.check(c.lib.ugsm_submit_full(c.handle, 1, pL, pR, W, H, L.strides[0], d_out))
        n = c.point_cloud(d_out, d_out + plane, d_out + 2 * plane, pL, W, H, L.strides[0], P1, P2, lib.cloud_params(), d_pts, n_all, d_cnt,
                          slot=1)
        assert n == n_all
        cn.assert_cloud_equal(c.cloud_to_host(d_pts, n), cn.records(xyz, word), "16 MP dense PCL32 after submit_full")
        zf = xyz[2][np.isfinite(xyz[2])]
        kw = dict(min_conf=0.25, z_min=float(np.percentile(zf, 5)), z_max=float(np.percentile(zf, 95)))
        exp = cn.records(xyz, word, conf=full[2], compact=True, **kw)
        assert 0 < exp.size < n_all
        raw = []
        for _ in range(2):
            n = c.point_cloud(d_out, d_out + plane, d_out + 2 * plane, pL, W, H, L.strides[0], P1, P2, lib.cloud_params(compact=True, **kw),
                              d_pts, n_all, d_cnt, slot=1)
            assert n == exp.size
            raw.append(c.to_host(d_pts, (n * 32,), np.uint8))
        assert np.array_equal(raw[0], raw[1]), "two compact runs differ"
        cn.assert_cloud_equal(raw[0].view(cn.DT_PCL32), exp, "16 MP compact PCL32")
        n = c.point_cloud(d_out, d_out + plane, d_out + 2 * plane, pL, W, H, L.strides[0], P1, P2,
                          lib.cloud_params(sampling=2, format=lib.UGSM_CLOUD_XYZRGB16), d_pts, n_all, d_cnt, slot=0)
        cn.assert_cloud_equal(c.cloud_to_host(d_pts, n, lib.UGSM_CLOUD_XYZRGB16), cn.records(xyz, word, s=2, fmt=cn.XYZRGB16),
                              "16 MP dense 16-byte, sampling 2")
        for p in (pL, pR, d_out, d_pts, d_cnt):
            c.free(p)
    finally:
        c.close()


def test_foveated_cloud_on_the_16mp_stack(lib, ctx, orc, oracle_16mp):
    """ugsm_point_cloud_fovea at src_level 0, 3 and 6 of the oracle's 16 MP fovea stack with ugsm_fovea_mapping's margins (the colour
    lookup inside the image, unclamped there), dense and compact; then margins pushed past the image edge, where the clamp acts."""
    g = oracle_16mp
    W, H, L, stack = g["W"], g["H"], g["L"], g["stack"]
    _, F, fh, fw = stack.shape
    sx, sy, sc = (np.ascontiguousarray(stack[k]) for k in range(3))
    dptr = [ctx.to_device(a) for a in (sx, sy, sc, L)]
    n_all = fw * fh
    d_pts = ctx.alloc(n_all * 32 + 4096)
    d_cnt = ctx.alloc(8)
    try:
        cases = [(src, *lib.fovea_mapping(W, H, src)) for src in (0, 3, 6)]
        l6, u6, s6 = cases[-1][1:]
        cases.append((6, l6 + 400, u6 - 2000, s6))      # past the right and the top edge
        cases.append((2, -300, 2900, lib.fovea_mapping(W, H, 2)[2]))
        for k, (src, left, upper, scale) in enumerate(cases):
            fired = cn.fovea_colour_at(W, H, fw, fh, left, upper, scale)[2]
            assert fired == (k >= 3)
            for fmt, compact, kw in ((cn.PCL32, False, {}), (cn.XYZRGB16, True, dict(min_conf=0.2))):
                exp = cn.cloud_fovea(orc, sx, sy, src, left, upper, scale, L, P1, P2, stackc=sc, fmt=fmt, compact=compact, **kw)
                n = ctx.point_cloud_fovea(dptr[0], dptr[1], dptr[2], fw, fh, src, left, upper, scale, dptr[3], W, H, L.strides[0], P1, P2,
                                          lib.cloud_params(format=fmt, compact=compact, **kw), d_pts, n_all, d_cnt)
                assert n == exp.size
                cn.assert_cloud_equal(ctx.cloud_to_host(d_pts, n, fmt), exp, f"fovea level {src} at ({left}, {upper}) fmt={fmt} compact={compact}")
    finally:
        for p in dptr + [d_pts, d_cnt]:
            ctx.free(p)


def test_bad_arguments_on_a_live_context(lib, ctx):
    """Every refusal of the host test, made on a live context with real buffers (large enough that nothing could be touched out of
    bounds even if a check were missing); then a call that passes."""
    W, H = 64, 32
    bufs = dict(dx=ctx.alloc(W * H * 4), dy=ctx.alloc(W * H * 4), conf=ctx.alloc(W * H * 4), rgb=ctx.alloc(3 * W * H),
                points=ctx.alloc(8192), count=ctx.alloc(8))
    so = lib.load()
    P = (C.c_double * 12)(*P1.reshape(12))

    def call(fovea, **over):
        a = dict(bufs, W=W, H=H, stride=3 * W, P1=P, P2=P, p=lib.cloud_params(), cap=100)
        if "points" in over and over["points"] is not None and over["points"] < 0x100000:
            over["points"] = bufs["points"] + 8       # (the misaligned case)
        a.update(over)
        p = C.byref(a["p"]) if a["p"] is not None else None
        if fovea:
            return so.ugsm_point_cloud_fovea(ctx.handle, 0, a["dx"], a["dy"], a["conf"], 40, 20, 0, 8, 6, C.c_float(1.0), a["rgb"], a["W"],
                                             a["H"], a["stride"], a["P1"], a["P2"], p, a["points"], a["cap"], a["count"])
        return so.ugsm_point_cloud(ctx.handle, 0, a["dx"], a["dy"], a["conf"], a["rgb"], a["W"], a["H"], a["stride"], a["P1"], a["P2"], p,
                                   a["points"], a["cap"], a["count"])
    try:
        for name, over in bad_argument_cases(lib):
            for fovea in (False, True):
                assert call(fovea, **dict(over)) == lib.UGSM_ERR_BAD_ARG, (name, fovea)
        assert so.ugsm_point_cloud(ctx.handle, 5, bufs["dx"], bufs["dy"], None, bufs["rgb"], W, H, 3 * W, P, P, C.byref(lib.cloud_params()),
                                   bufs["points"], 100, bufs["count"]) == lib.UGSM_ERR_BAD_ARG   # (no such slot)
        ctx.check(so.ugsm_wait(ctx.handle, 0))
        assert call(False) == lib.UGSM_OK and call(True) == lib.UGSM_OK
        ctx.check(so.ugsm_wait(ctx.handle, 0))
    finally:
        for p in bufs.values():
            ctx.free(p)
