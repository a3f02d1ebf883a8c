"""The depth image on the device (ugsm_depth_image, ugsm_depth_image_fovea, ugsm_match_full_depth; REP 118 32FC1 / 16UC1) against the library's
own planes and resized clouds and against the numpy restatement (tests/depth_np.py).  Everything is bit for bit, the NaN's payload included.

Every call here runs on caller-owned memory between guard bands (tests/guarded.py for the float planes; _Band for the image, whose element
may be two bytes): a byte written in front of a buffer or behind it, or into an input, fails the case.  Every 16U and every filtered case
asserts on its EXPECTED image that at least 25 % of the pixels are valid and at least 5 % are not (depth_np.assert_both_branches): a kernel
that stores all-invalid cannot pass.  The shapes are the smallest at which the flat runs can go wrong: 67 x 41 (odd width: 16U rows on 2-byte
boundaries, a head and a tail), 8 x 3 (shorter than a wave's runs), 1 x 1, 255 x 2, 64 x 48."""
import ctypes as C

import numpy as np
import pytest

import depth_np as dn
import resize_np as rn
from guarded import POISON, Guards
from test_depth_host import bad_argument_cases, call, resolve
from test_gpu_cloud import P1, P2, P2A

pytestmark = pytest.mark.gpu

SHAPES = [(67, 41), (8, 3), (1, 1), (255, 2), (64, 48)]
WILD = (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40)
BAND = 4096          # poisoned bytes on either side of an image
FW, FH, FLV, FF = 160, 120, 8, 4   # the fovea cases' frame, levels and fovea levels


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


@pytest.fixture(scope="module")
def fctx(lib):
    c = lib.Context(levels=FLV, fovea_levels=FF)
    yield c
    c.close()


class _Band:
    """`nbytes` of device memory at base + BAND + shift (the base 16-byte aligned) between two bands of POISON bytes."""

    def __init__(self, ctx, nbytes, shift):
        self.ctx, self.n, self.lo = ctx, nbytes, BAND + shift
        self.base = ctx.to_device(np.full(2 * BAND + shift + nbytes, POISON, np.uint8))
        assert self.base % 16 == 0
        self.ptr = self.base + self.lo

    def read(self, dtype, shape, what):
        raw = self.ctx.to_host(self.base, (2 * BAND + (self.lo - BAND) + self.n,), np.uint8)
        assert (raw[:self.lo] == POISON).all(), f"{what}: bytes in front of the image were written"
        assert (raw[self.lo + self.n:] == POISON).all(), f"{what}: bytes behind the image were written"
        return raw[self.lo:self.lo + self.n].copy().view(dtype).reshape(shape)

    def free(self):
        self.ctx.free(self.base)


def field(W, H, seed=0, wild=80):
    """Smooth-ish disparities around the rig's, and the cloud tests' hard values in dx and in the confidence: each of them at one pixel in
    `wild` (0: none)."""
    rng = np.random.Generator(np.random.PCG64(W * 7919 + H * 31 + seed))
    dx = rng.normal(-40, 12, (H, W)).astype(np.float32)
    dy = rng.normal(0, 2, (H, W)).astype(np.float32)
    conf = rng.uniform(0, 1, (H, W)).astype(np.float32)
    if wild and W * H >= 16:
        for a, vals in ((dx, WILD), (conf, (np.nan, np.inf, -np.inf))):
            for v in vals:
                a.flat[rng.integers(0, a.size, max(1, a.size // wild))] = v
    return dx, dy, conf


def window(z, lo=15, hi=85):
    """A Z window from the restatement's own Z: the lo-th and hi-th percentile of its finite values."""
    zf = z[np.isfinite(z)]
    return float(np.percentile(zf, lo)), float(np.percentile(zf, hi))


def run(ctx, lib, dx, dy, conf, W, H, P2_, params, in_shift=0, out_shift=0, what=""):
    """ugsm_depth_image on guarded buffers -> (image, valid count)."""
    dw, dh = lib.depth_image_size(W, H, params.factor)
    dtype = lib.DEPTH_DTYPES[params.format]
    g, band = Guards(ctx), _Band(ctx, dw * dh * dtype.itemsize, out_shift)
    d_valid = ctx.to_device(np.full(1, 0xDEADBEEF, np.uint64))
    try:
        ddx, ddy = g.inp(dx, in_shift), g.inp(dy, in_shift)
        dconf = g.inp(conf, in_shift) if conf is not None else None
        n = ctx.depth_image(ddx, ddy, dconf, W, H, P1, P2_, params, band.ptr, d_valid)
        return band.read(dtype, (dh, dw), what), n
    finally:
        g.done(what)
        band.free()
        ctx.free(d_valid)


@pytest.mark.parametrize("W,H", SHAPES)
def test_default_32f_is_the_z_plane_of_triangulate(lib, ctx, orc, W, H):
    """32F with the default parameters: every finite Z equals ugsm_triangulate's plane 2 bit for bit, the rest is the NaN 0x7FC00000 -- at
    16-byte bases and at 4-byte ones."""
    dx, dy, _ = field(W, H)
    if (W, H) == (1, 1):
        dx[0, 0] = -37.5
    d = [ctx.to_device(a) for a in (dx, dy)]
    d_xyz = ctx.alloc(3 * W * H * 4)
    try:
        ctx.triangulate(d[0], d[1], W, H, P1, P2A, d_xyz)
        z = ctx.to_host(d_xyz, (3, H, W))[2]
    finally:
        for p in d + [d_xyz]:
            ctx.free(p)
    exp = np.where(np.isfinite(z), z.view(np.uint32), dn.QNAN).astype(np.uint32).view(np.float32)
    for in_shift, out_shift in ((0, 0), (1, 4), (3, 12)):
        got, n = run(ctx, lib, dx, dy, None, W, H, P2A, lib.depth_params(), in_shift, out_shift, f"{W}x{H} shifts {in_shift}/{out_shift}")
        dn.assert_image_equal(got, exp, f"32F default vs ugsm_triangulate, {W}x{H}, shifts {in_shift}/{out_shift}")
        assert n == int(np.isfinite(z).sum())
    dn.assert_image_equal(exp, dn.depth_image(orc, dx, dy, P1, P2A)[0], f"the restatement, {W}x{H}")
    if W * H >= 16:
        assert np.isnan(exp).any() and np.isfinite(exp).any()


def filtered_cases(orc, W, H):
    """The filtered and the 16U cases of a shape: (label, dx, dy, conf, P2, keyword arguments of depth_params / depth_np)."""
    dx, dy, conf = field(W, H)
    z = orc.triangulate(dx, dy, P1, P2)[2]
    zlo, zhi = window(z)
    za = orc.triangulate(dx, dy, P1, P2A)[2]
    alo, ahi = window(za, 20, 90)
    pos = z[np.isfinite(z) & (z > 0)]
    unit = 60.0 / float(np.percentile(pos, 80))          # the farthest fifth of the rig's depths lies past 65.535 m
    return [("32F window", dx, dy, conf, P2, dict(fmt=dn.FMT_32F, unit=0.5, z_min=zlo, z_max=zhi)),
            ("32F window + conf", dx, dy, conf, P2A, dict(fmt=dn.FMT_32F, unit=2.0, z_min=alo, z_max=ahi, min_conf=0.2)),
            ("32F conf only", dx, dy, conf, P2, dict(fmt=dn.FMT_32F, min_conf=0.4)),
            ("16U unit", dx, dy, None, P2, dict(fmt=dn.FMT_16U, unit=unit)),
            ("16U window + conf", dx, dy, conf, P2, dict(fmt=dn.FMT_16U, unit=unit / 2, z_min=zlo, z_max=zhi, min_conf=0.1))]


def params_of(lib, kw, factor=1.0):
    kw = dict(kw)
    return lib.depth_params(format=kw.pop("fmt"), factor=factor, **kw)


@pytest.mark.parametrize("W,H", [s for s in SHAPES if s != (1, 1)])
def test_filtered_and_16u_images_match_the_restatement(lib, ctx, orc, W, H):
    """32F and 16U with unit, z_min / z_max and min_conf; d_valid is the restatement's count.  Inputs at a 4-byte base that is not 16-byte
    aligned, the image at a 2-byte (16U) / 4-byte (32F) base that is not wider-aligned, and both aligned."""
    for label, dx, dy, conf, P2_, kw in filtered_cases(orc, W, H):
        exp, valid = dn.depth_image(orc, dx, dy, P1, P2_, conf=conf, **kw)
        dn.assert_both_branches(valid, f"{label} {W}x{H}")
        size = exp.dtype.itemsize
        for in_shift, out_shift in ((0, 0), (1, size), (3, 16 - size), (2, 3 * size)):
            what = f"{label}, {W}x{H}, shifts {in_shift}/{out_shift}"
            got, n = run(ctx, lib, dx, dy, conf, W, H, P2_, params_of(lib, kw), in_shift, out_shift, what)
            dn.assert_image_equal(got, exp, what)
            assert n == int(valid.sum()), what


def test_one_pixel_images(lib, ctx, orc):
    """1 x 1: one pixel cannot show both branches, so eight one-pixel fields do together."""
    flags = []
    for seed, d in enumerate((-37.5, -12.0, 5.0, np.nan, -80.0, np.inf, -20.0, -55.0)):
        dx, dy = np.full((1, 1), d, np.float32), np.full((1, 1), 0.25, np.float32)
        conf = np.full((1, 1), 0.1 * seed, np.float32)
        kw = dict(fmt=dn.FMT_16U, unit=1.0, min_conf=0.05)
        exp, valid = dn.depth_image(orc, dx, dy, P1, P2, conf=conf, **kw)
        flags.append(bool(valid[0, 0]))
        for out_shift in (0, 2, 14):
            got, n = run(ctx, lib, dx, dy, conf, 1, 1, P2, params_of(lib, kw), 1, out_shift, f"1x1 field {seed}")
            dn.assert_image_equal(got, exp, f"1x1 field {seed} shift {out_shift}")
            assert n == int(valid.sum())
    dn.assert_both_branches(np.array(flags), "the one-pixel fields together")


@pytest.mark.parametrize("factor", [0.2, 0.5, 1.0])
def test_resized_image_is_the_z_of_the_resized_cloud(lib, ctx, orc, factor):
    """67 x 41 at factor 0.2, 0.5 and 1: the image equals the z field of ugsm_point_cloud_resized's dense records, rearranged from the
    cloud's column-major order, and equals the restatement; the filtered forms against the restatement."""
    W, H = 67, 41
    dx, dy, conf = field(W, H, wild=700)       # (a wild value spoils the sixteen pixels of every footprint it lies in)
    rgb = np.zeros((H, W, 3), np.uint8)
    dw, dh = lib.depth_image_size(W, H, factor)
    dptr = [ctx.to_device(a) for a in (dx, dy, conf, rgb)]
    d_pts, d_cnt = ctx.alloc(dw * dh * 32), ctx.alloc(8)
    try:
        n = ctx.point_cloud_resized(*dptr, W, H, 3 * W, P1, P2A, factor, lib.cloud_params(), d_pts, dw * dh, d_cnt)
        assert n == dw * dh
        zc = ctx.cloud_to_host(d_pts, n)["z"].reshape(dw, dh).T
    finally:
        for p in dptr + [d_pts, d_cnt]:
            ctx.free(p)
    exp = np.where(np.isfinite(zc), zc.view(np.uint32), dn.QNAN).astype(np.uint32).view(np.float32)
    got, nv = run(ctx, lib, dx, dy, None, W, H, P2A, lib.depth_params(factor=factor), 1, 4, f"resized {factor}")
    dn.assert_image_equal(got, exp, f"32F default vs the resized cloud's z, factor {factor}")
    assert nv == int(np.isfinite(zc).sum())
    dn.assert_image_equal(got, dn.depth_image(orc, dx, dy, P1, P2A, factor=factor)[0], f"32F default vs the restatement, factor {factor}")
    z = rn.resize_cubic(orc.triangulate(dx, dy, P1, P2)[2], dw, dh)
    zlo, zhi = window(z, 20, 80)
    unit = 60.0 / float(np.percentile(z[np.isfinite(z) & (z > 0)], 80))
    for kw, c in ((dict(fmt=dn.FMT_16U, unit=unit), None), (dict(fmt=dn.FMT_16U, unit=unit / 2, z_min=zlo, z_max=zhi, min_conf=0.1), conf),
                  (dict(fmt=dn.FMT_32F, unit=3.0, z_min=zlo, z_max=zhi, min_conf=0.2), conf)):
        exp, valid = dn.depth_image(orc, dx, dy, P1, P2, conf=c, factor=factor, **kw)
        dn.assert_both_branches(valid, f"factor {factor} {kw}")
        for in_shift, out_shift in ((0, 0), (3, exp.dtype.itemsize)):
            got, nv = run(ctx, lib, dx, dy, c, W, H, P2, params_of(lib, kw, factor), in_shift, out_shift, f"resized {factor} {kw}")
            dn.assert_image_equal(got, exp, f"factor {factor} {kw} shifts {in_shift}/{out_shift}")
            assert nv == int(valid.sum())


# ---- the fovea form ------------------------------------------------------------------------------------------------------------------------

def stacks(lib, seed=0):
    fw, fh = lib.fovea_dims(FW, FH, FLV, FF)
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    sx = rng.normal(-12, 4, (FF, fh, fw)).astype(np.float32)      # finite and far inside the range of int
    sy = rng.normal(0, 1.5, (FF, fh, fw)).astype(np.float32)
    sc = rng.uniform(0, 1, (FF, fh, fw)).astype(np.float32)
    sc.flat[rng.integers(0, sc.size, sc.size // 60)] = np.nan
    return fw, fh, sx, sy, sc


def run_fovea(fctx, lib, sx, sy, sc, off, level, params, in_shift=0, out_shift=0, what=""):
    fw, fh = sx.shape[2], sx.shape[1]
    dw, dh = lib.depth_image_size(fw, fh, params.factor)
    nl = FF if level == lib.UGSM_DEPTH_ALL_LEVELS else 1
    dtype = lib.DEPTH_DTYPES[params.format]
    g, band = Guards(fctx), _Band(fctx, nl * dw * dh * dtype.itemsize, out_shift)
    d_valid = fctx.to_device(np.full(nl, 0xDEADBEEF, np.uint64))
    try:
        dsx, dsy = g.inp(sx, in_shift), g.inp(sy, in_shift)
        dsc = g.inp(sc, in_shift) if sc is not None else None
        counts = fctx.depth_image_fovea(dsx, dsy, dsc, FW, FH, off, level, P1, P2, params, band.ptr, d_valid)
        return band.read(dtype, (nl, dh, dw), what), counts
    finally:
        g.done(what)
        band.free()
        fctx.free(d_valid)


@pytest.mark.parametrize("off", [(0, 0), (13, -9)])
def test_fovea_levels_match_triangulate_fovea_and_all_levels_match_the_single_ones(lib, fctx, orc, off):
    """One level against ugsm_triangulate_fovea with ugsm_fovea_level_mapping's numbers; UGSM_DEPTH_ALL_LEVELS against the per-level calls
    (the images laid out as stackH is, level 0 first) with its F counts; filtered 16U and resized forms against the restatement."""
    fw, fh, sx, sy, sc = stacks(lib, off[0])
    ALL = lib.UGSM_DEPTH_ALL_LEVELS
    maps = [lib.fovea_level_mapping(FW, FH, FLV, FF, k, off) for k in range(FF)]
    d = [fctx.to_device(a) for a in (sx, sy)]
    d_xyz = fctx.alloc(3 * fw * fh * 4)
    per_level = []
    try:
        for k in range(FF):
            fctx.triangulate_fovea(d[0], d[1], fw, fh, k, *maps[k], P1, P2, d_xyz)
            z = fctx.to_host(d_xyz, (3, fh, fw))[2]
            assert np.isfinite(z).all()
            got, counts = run_fovea(fctx, lib, sx, sy, None, off, k, lib.depth_params(), 1, 4, f"fovea level {k}")
            dn.assert_image_equal(got[0], z, f"fovea level {k} off {off} vs ugsm_triangulate_fovea")
            assert counts == [fw * fh]
            per_level.append(got[0])
    finally:
        for p in d + [d_xyz]:
            fctx.free(p)
    got, counts = run_fovea(fctx, lib, sx, sy, None, off, ALL, lib.depth_params(), 3, 12, "all levels 32F")
    dn.assert_image_equal(got, np.stack(per_level), f"all levels vs the per-level calls, off {off}")
    assert counts == [fw * fh] * FF
    zs = np.stack([orc.triangulate_fovea(sx, sy, k, *maps[k], P1, P2)[2] for k in range(FF)])
    zlo, zhi = window(zs, 10, 80)
    unit = 60.0 / float(np.percentile(zs[zs > 0], 85))
    for factor in (1.0, 0.5):
        for kw in (dict(fmt=dn.FMT_16U, unit=unit, min_conf=0.15), dict(fmt=dn.FMT_32F, unit=0.25, z_min=zlo, z_max=zhi, min_conf=0.1)):
            exp = [dn.depth_image_fovea(orc, sx, sy, k, *maps[k], P1, P2, stackc=sc, factor=factor, **kw) for k in range(FF)]
            dn.assert_both_branches(np.stack([v for _, v in exp]), f"fovea {kw} factor {factor}")
            size = exp[0][0].dtype.itemsize
            got, counts = run_fovea(fctx, lib, sx, sy, sc, off, ALL, params_of(lib, kw, factor), 1, size, f"all levels {kw} factor {factor}")
            dn.assert_image_equal(got, np.stack([e for e, _ in exp]), f"all levels {kw} factor {factor} off {off}")
            assert counts == [int(v.sum()) for _, v in exp]
            k = 2
            got, counts = run_fovea(fctx, lib, sx, sy, sc, off, k, params_of(lib, kw, factor), 3, 3 * size, f"level {k} {kw} factor {factor}")
            dn.assert_image_equal(got[0], exp[k][0], f"level {k} {kw} factor {factor} off {off}")
            assert counts == [int(exp[k][1].sum())]


# ---- the blocking call ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mono", [False, True])
def test_match_full_depth_is_match_full_then_depth_image(lib, orc, mono):
    """64 x 48, levels 5, rgb8 and mono8: the image equals ugsm_match_full followed by ugsm_depth_image on its planes -- with the three
    plane pointers NULL and with all given, when the planes equal ugsm_match_full's too."""
    from ug_stereomatcher_amd import synth
    P2M = P1.copy()          # the rig mirrored: the synthetic pairs' disparities are positive, and Z > 0 needs the baseline on that side
    P2M[0, 3] = 7.3230899280915291e+03 * 0.12
    W, H = 64, 48
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 7)
    if mono:
        L, R = np.ascontiguousarray(L[..., 1]), np.ascontiguousarray(R[..., 1])
    with lib.Context(levels=5) as c:
        if mono:
            c.set_input_format(lib.UGSM_INPUT_MONO8)
        planes = np.empty((3, H, W), np.float32)
        c.check(c.lib.ugsm_match_full(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], *(planes[k].ctypes.data for k in range(3))))
        z = orc.triangulate(planes[0], planes[1], P1, P2M)[2]
        zlo, zhi = window(z, 20, 90)
        unit = 60.0 / float(np.percentile(z[np.isfinite(z) & (z > 0)], 80))
        for kw in (dict(fmt=dn.FMT_32F), dict(fmt=dn.FMT_16U, unit=unit, min_conf=0.05), dict(fmt=dn.FMT_32F, z_min=zlo, z_max=zhi, factor=0.5)):
            factor = kw.pop("factor", 1.0)
            prm = params_of(lib, kw, factor)
            want, _ = run(c, lib, planes[0], planes[1], planes[2], W, H, P2M, prm, what=f"depth of the planes {kw}")
            exp, valid = dn.depth_image(orc, planes[0], planes[1], P1, P2M, conf=planes[2], factor=factor, **kw)
            if kw != dict(fmt=dn.FMT_32F):
                dn.assert_both_branches(valid, f"match_full_depth {kw}")
            dn.assert_image_equal(want, exp, f"ugsm_depth_image of the planes vs the restatement {kw}")
            alone = c.match_full_depth(L, R, P1, P2M, prm)
            dn.assert_image_equal(alone, want, f"ugsm_match_full_depth, no planes, mono={mono} {kw}")
            both, out = c.match_full_depth(L, R, P1, P2M, prm, planes=True)
            dn.assert_image_equal(both, want, f"ugsm_match_full_depth, with planes, mono={mono} {kw}")
            assert np.array_equal(out.view(np.uint32), planes.view(np.uint32))
        # one plane alone comes down where only it is asked for
        depth, only = np.empty((H, W), np.float32), np.full((H, W), -1.0, np.float32)
        P = [(C.c_double * 12)(*np.asarray(p, np.float64).reshape(12)) for p in (P1, P2M)]
        c.check(c.lib.ugsm_match_full_depth(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], P[0], P[1], C.byref(lib.depth_params()),
                                            depth.ctypes.data, None, None, only.ctypes.data))
        assert np.array_equal(only.view(np.uint32), planes[2].view(np.uint32))
        want16 = c.match_full_depth(L, R, P1, P2M, lib.depth_params(format=lib.UGSM_DEPTH_16U, unit=unit))
    if mono:
        return
    # the Python MatchGPULib's depthImage is that call (the class takes rgb8 and float images: it sets the input format from the array)
    from ug_stereomatcher_amd import MatchGPULib
    m = MatchGPULib(levels=5)
    try:
        got16, fin = m.depthImage(L, R, P1, P2M, "16UC1", unit=unit, planes=True)
        dn.assert_image_equal(got16, want16, f"MatchGPULib.depthImage 16UC1, mono={mono}")
        assert np.array_equal(fin.view(np.uint32), planes.view(np.uint32))
        with pytest.raises(lib.UgsmError):
            m.depthImage(L, R, P1, P2M, "8UC1")
    finally:
        m.close()


# ---- the refusals on a live context -------------------------------------------------------------------------------------------------------

def test_bad_arguments_on_a_live_context_write_nothing(lib, fctx):
    """Every refusal of the three entry points on a live context with real buffers: UGSM_ERR_BAD_ARG, the image and the count untouched;
    then calls that pass."""
    fw, fh = lib.fovea_dims(FW, FH, FLV, FF)
    W, H = 64, 48
    n = max(W * H, FF * fw * fh)
    bufs = dict(dx=fctx.alloc(n * 4), dy=fctx.alloc(n * 4), conf=fctx.alloc(n * 4), depth=fctx.to_device(np.full(n * 4, POISON, np.uint8)),
                valid=fctx.to_device(np.full(FF, 0xDEADBEEF, np.uint64)))
    L = np.zeros((H, W, 3), np.uint8)
    host = np.full(W * H, -3.0, np.float32)

    def untouched():
        fctx.check(fctx.lib.ugsm_wait(fctx.handle, 0))
        return ((fctx.to_host(bufs["depth"], (n * 4,), np.uint8) == POISON).all()
                and (fctx.to_host(bufs["valid"], (FF,), np.uint64) == 0xDEADBEEF).all() and (host == -3.0).all())
    try:
        for name in ("ugsm_depth_image", "ugsm_depth_image_fovea", "ugsm_match_full_depth"):
            live = dict(bufs, ctx=fctx.handle)
            if name == "ugsm_depth_image_fovea":
                live.update(W=FW, H=FH)
            if name == "ugsm_match_full_depth":
                live.update(L=L.ctypes.data, R=L.ctypes.data, depth=host.ctypes.data)
            for label, over in bad_argument_cases(lib, name):
                a = dict(live)
                a.update(resolve(over, bufs))
                assert call(lib, name, **a) == lib.UGSM_ERR_BAD_ARG, (name, label)
            assert untouched(), name
        assert call(lib, "ugsm_depth_image_fovea", **dict(bufs, ctx=fctx.handle, W=FW, H=FH, level=FF)) == lib.UGSM_ERR_BAD_ARG
        with lib.Context(levels=5, fovea_levels=1) as c1:     # the fovea form needs a stack of at least two levels
            assert call(lib, "ugsm_depth_image_fovea", **dict(bufs, ctx=c1.handle, W=FW, H=FH)) == lib.UGSM_ERR_BAD_ARG
        assert untouched()
        for key, value in (("dx", -30.0), ("dy", 0.0), ("conf", 1.0)):
            plane = np.full(n, value, np.float32)             # (held while the copy reads it)
            fctx.check(fctx.lib.ugsm_copy_to_device(fctx.handle, bufs[key], plane.ctypes.data, n * 4))
        rig = dict(P1=(C.c_double * 12)(*P1.reshape(12)), P2=(C.c_double * 12)(*P2.reshape(12)))     # (a finite Z everywhere)
        assert call(lib, "ugsm_depth_image", **dict(bufs, ctx=fctx.handle, **rig)) == lib.UGSM_OK
        fctx.check(fctx.lib.ugsm_wait(fctx.handle, 0))
        assert fctx.to_host(bufs["valid"], (1,), np.uint64)[0] == W * H
        assert call(lib, "ugsm_depth_image_fovea", **dict(bufs, ctx=fctx.handle, W=FW, H=FH, level=lib.UGSM_DEPTH_ALL_LEVELS, **rig)) == lib.UGSM_OK
        fctx.check(fctx.lib.ugsm_wait(fctx.handle, 0))
        assert fctx.to_host(bufs["valid"], (FF,), np.uint64).tolist() == [fw * fh] * FF
    finally:
        for p in bufs.values():
            fctx.free(p)


def test_depth_calls_are_refused_while_enqueued_pairs_are_outstanding(lib):
    """UGSM_ERR_STATE: a pair outstanding in the queue makes the slots the queue's; nothing is written, and after the drain the calls work."""
    from ug_stereomatcher_amd import synth
    L, R, _, _ = synth.make_pair(FW, FH, synth.BASE_SEED + 9)
    fw, fh = lib.fovea_dims(FW, FH, FLV, FF)
    n = max(FW * FH, FF * fw * fh)
    rig = dict(P1=(C.c_double * 12)(*P1.reshape(12)), P2=(C.c_double * 12)(*P2.reshape(12)))
    with lib.Context(levels=FLV, fovea_levels=FF, slots=2) as c:
        dL, dR, d_out = c.to_device(L), c.to_device(R), c.alloc(3 * FW * FH * 4)
        plane = np.full(n, -30.0, np.float32)
        bufs = dict(dx=c.to_device(plane), dy=c.to_device(np.zeros(n, np.float32)), conf=c.to_device(np.ones(n, np.float32)),
                    depth=c.to_device(np.full(n * 4, POISON, np.uint8)), valid=c.to_device(np.full(FF, 0xDEADBEEF, np.uint64)))
        full = dict(bufs, ctx=c.handle, W=FW, H=FH, **rig)
        try:
            c.enqueue_full(dL, dR, FW, FH, L.strides[0], d_out, 7)
            assert call(lib, "ugsm_depth_image", **full) == lib.UGSM_ERR_STATE
            assert b"queue" in c.lib.ugsm_last_error(c.handle)
            assert call(lib, "ugsm_depth_image_fovea", **dict(full, level=lib.UGSM_DEPTH_ALL_LEVELS)) == lib.UGSM_ERR_STATE
            done = c.drain()
            assert [int(d.tag) for d in done] == [7] and done[0].status == 0
            assert (c.to_host(bufs["depth"], (n * 4,), np.uint8) == POISON).all()
            assert (c.to_host(bufs["valid"], (FF,), np.uint64) == 0xDEADBEEF).all()
            assert call(lib, "ugsm_depth_image", **full) == lib.UGSM_OK
            c.check(c.lib.ugsm_wait(c.handle, 0))
            assert c.to_host(bufs["valid"], (1,), np.uint64)[0] == FW * FH
        finally:
            for p in list(bufs.values()) + [dL, dR, d_out]:
                c.free(p)


def test_images_larger_than_one_pass_of_the_grid(lib, ctx, orc):
    """A depth launch holds at most 2048 workgroups of 256 runs a level, and a workgroup walks on by the grid's width: 2049 x 1031 (32F, 528 k
    runs of four pixels) and 2049 x 2057 (16U, 527 k runs of eight) are the smallest odd-width images whose last runs come in a second pass.
    32F against ugsm_triangulate's plane, 16U against the restatement, with the counts."""
    W, H = 2049, 1031
    dx, dy, _ = field(W, H)
    d = [ctx.to_device(a) for a in (dx, dy)]
    d_xyz = ctx.alloc(3 * W * H * 4)
    try:
        ctx.triangulate(d[0], d[1], W, H, P1, P2, d_xyz)
        z = ctx.to_host(d_xyz, (3, H, W))[2]
    finally:
        for p in d + [d_xyz]:
            ctx.free(p)
    exp = np.where(np.isfinite(z), z.view(np.uint32), dn.QNAN).astype(np.uint32).view(np.float32)
    got, n = run(ctx, lib, dx, dy, None, W, H, P2, lib.depth_params(), 1, 4, "2049 x 1031 32F")
    dn.assert_image_equal(got, exp, "32F default vs ugsm_triangulate, 2049 x 1031")
    assert n == int(np.isfinite(z).sum())
    W, H = 2049, 2057
    dx, dy, conf = field(W, H)
    z = orc.triangulate(dx, dy, P1, P2)[2]
    kw = dict(fmt=dn.FMT_16U, unit=60.0 / float(np.percentile(z[np.isfinite(z) & (z > 0)], 80)), min_conf=0.1)
    exp, valid = dn.convert(z, conf=conf, **kw)
    dn.assert_both_branches(valid, "2049 x 2057 16U")
    got, n = run(ctx, lib, dx, dy, conf, W, H, P2, params_of(lib, kw), 3, 6, "2049 x 2057 16U")
    dn.assert_image_equal(got, exp, "16U vs the restatement, 2049 x 2057")
    assert n == int(valid.sum())
