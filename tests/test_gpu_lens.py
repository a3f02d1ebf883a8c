"""Lens distortion on the device (ugsm_set_lens; include/ugsm.h, "lens distortion"): every call that honours the lens against the numpy
restatement (tests/lens_np.py under tests/cloud_np.py, resize_np.py, depth_np.py and stack_cloud_np.py) bit for bit, a NaN X, Y or Z equal to
any NaN; a zero-D lens and a cleared lens against the calls without one; the capture of the setting by a call; the refusals.

Planes of 97 x 131 (more than three 32-column tiles and two 64-row tiles, ragged both ways); the fovea cases on a 160 x 120 frame with 8
levels, 3 fovea levels and an off-centre window.  Random fields with the hard values of tests/test_gpu_depth.py in dx and a NaN-sprinkled
confidence; the fovea stacks are finite (their right position is truncated to int) with a NaN-sprinkled confidence."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import depth_np as dn
import lens_np as ln
import resize_np as rn
import stack_cloud_np as sn
from test_gpu_cloud import POISON, _poisoned, _read

pytestmark = pytest.mark.gpu

W, H = 97, 131
FW, FH, FLV, FF, OFF = 160, 120, 8, 3, (13, -9)
WILD = (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40)
F32 = np.float32
PCL32, XYZ16 = cn.PCL32, cn.XYZRGB16


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(levels=FLV, fovea_levels=FF)
    yield c
    c.close()


class Data:
    """The inputs of every case, on the host and on the device, and the parameters the filtered cases share."""

    def __init__(self, ctx, lib):
        rig = ln.rigs()["small"]
        self.rig, self.P1, self.P2 = rig, rig["P1"], rig["P2"]
        rng = np.random.Generator(np.random.PCG64(4242))
        self.dx = rng.normal(-40, 12, (H, W)).astype(F32)
        self.dy = rng.normal(0, 2, (H, W)).astype(F32)
        self.conf = rng.uniform(0, 1, (H, W)).astype(F32)
        for a, vals in ((self.dx, WILD), (self.conf, (np.nan, np.inf, -np.inf))):
            for v in vals:
                a.flat[rng.integers(0, a.size, a.size // 80)] = v
        self.dxr = rng.normal(-40, 12, (H, W)).astype(F32)       # the resized cases: a hard value spoils the sixteen pixels of every footprint it lies in
        for v in WILD:
            self.dxr.flat[rng.integers(0, self.dxr.size, self.dxr.size // 700)] = v
        self.rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        self.fw, self.fh = lib.fovea_dims(FW, FH, FLV, FF)
        self.sx = rng.normal(-12, 4, (FF, self.fh, self.fw)).astype(F32)
        self.sy = rng.normal(0, 1.5, (FF, self.fh, self.fw)).astype(F32)
        self.sc = rng.uniform(0, 1, (FF, self.fh, self.fw)).astype(F32)
        self.sc.flat[rng.integers(0, self.sc.size, self.sc.size // 60)] = np.nan
        self.rgbF = rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)
        self.maps = [lib.fovea_level_mapping(FW, FH, FLV, FF, k, OFF) for k in range(FF)]
        assert self.maps == [sn.level_mapping(FW, FH, FF, k, OFF) for k in range(FF)]
        # the filtered cases' windows, from the restatement's own Z without a lens
        z = ln.triangulate(self.dx, self.dy, self.P1, self.P2)[2]
        zf = z[np.isfinite(z)]
        self.zwin = float(np.percentile(zf, 15)), float(np.percentile(zf, 85))
        zs = np.stack([ln.triangulate_fovea(self.sx, self.sy, k, *self.maps[k], self.P1, self.P2)[2] for k in range(FF)])
        self.zwin_f = float(np.percentile(zs, 10)), float(np.percentile(zs, 80))
        self.unit = 60.0 / float(np.percentile(zf[zf > 0], 85))   # 16U: the 85th percentile at 60 000
        self.ctx = ctx
        self.d = {k: ctx.to_device(getattr(self, k)) for k in ("dx", "dy", "conf", "dxr", "rgb", "sx", "sy", "sc", "rgbF")}

    def free(self):
        for p in self.d.values():
            self.ctx.free(p)


@pytest.fixture(scope="module")
def data(ctx, lib):
    d = Data(ctx, lib)
    yield d
    d.free()


# ---- the honoured calls: each case runs one call on the device and states it in numpy ---------------------------------------------------

def _cloud_call(ctx, lib, fmt, cap, call):
    """A cloud call into a poisoned buffer of cap + 64 records -> the records written; call(d_points, cap, d_count) -> the count."""
    d_pts = _poisoned(ctx, (cap + 64) * cn.DTYPES[fmt].itemsize)
    d_cnt = ctx.to_device(np.full(1, -7, np.int64))
    try:
        n = call(d_pts, cap, d_cnt)
        assert 0 <= n <= cap
        return _read(ctx, lib, d_pts, cap, 64, fmt, n)
    finally:
        ctx.free(d_pts)
        ctx.free(d_cnt)


def _depth_call(ctx, lib, params, pw, ph, levels, call):
    """A depth call into a poisoned buffer -> (images (levels, dh, dw), the valid counts); call(d_depth, d_valid) -> the counts."""
    dw, dh = lib.depth_image_size(pw, ph, params.factor)
    dtype = lib.DEPTH_DTYPES[params.format]
    nbytes = levels * dw * dh * dtype.itemsize
    d_img = _poisoned(ctx, nbytes + 256)
    d_valid = ctx.to_device(np.full(levels, 0xDEADBEEF, np.uint64))
    try:
        counts = call(d_img, d_valid)
        raw = ctx.to_host(d_img, (nbytes + 256,), np.uint8)
        assert (raw[nbytes:] == POISON).all(), "a byte behind the image was written"
        return raw[:nbytes].copy().view(dtype).reshape(levels, dh, dw), np.atleast_1d(np.array(counts, np.int64))
    finally:
        ctx.free(d_img)
        ctx.free(d_valid)


def _planes(ctx, n, call):
    d_xyz = _poisoned(ctx, 3 * n * 4 + 256)
    try:
        call(d_xyz)
        raw = ctx.to_host(d_xyz, (3 * n * 4 + 256,), np.uint8)
        assert (raw[3 * n * 4:] == POISON).all()
        return raw[:3 * n * 4].copy().view(F32)
    finally:
        ctx.free(d_xyz)


def case_tri(ctx, lib, D, lo):
    got = _planes(ctx, W * H, lambda o: ctx.triangulate(D.d["dx"], D.d["dy"], W, H, D.P1, D.P2, o))
    return [got.reshape(3, H, W)], [lo.triangulate(D.dx, D.dy, D.P1, D.P2)]


def case_tri_fovea(level):
    def case(ctx, lib, D, lo):
        got = _planes(ctx, D.fw * D.fh, lambda o: ctx.triangulate_fovea(D.d["sx"], D.d["sy"], D.fw, D.fh, level, *D.maps[level], D.P1, D.P2, o))
        return [got.reshape(3, D.fh, D.fw)], [lo.triangulate_fovea(D.sx, D.sy, level, *D.maps[level], D.P1, D.P2)]
    return case


def case_cloud(fmt, s, compact):
    def case(ctx, lib, D, lo):
        kw = dict(min_conf=0.2, z_min=D.zwin[0], z_max=D.zwin[1]) if compact else {}
        prm = lib.cloud_params(sampling=s, format=fmt, compact=compact, **kw)
        got = _cloud_call(ctx, lib, fmt, cn.cloud_points(W, H, s), lambda p, cap, c: ctx.point_cloud(
            D.d["dx"], D.d["dy"], D.d["conf"], D.d["rgb"], W, H, 3 * W, D.P1, D.P2, prm, p, cap, c))
        exp = cn.cloud(lo, D.dx, D.dy, D.rgb, D.P1, D.P2, conf=D.conf, s=s, fmt=fmt, compact=compact, **kw)
        if compact:
            assert 0.2 * W * H < exp.size < 0.8 * W * H        # (the filter keeps some and drops some)
        return [got], [exp]
    return case


def case_cloud_fovea(ctx, lib, D, lo):
    k = 1
    prm = lib.cloud_params(format=XYZ16)
    got = _cloud_call(ctx, lib, XYZ16, D.fw * D.fh, lambda p, cap, c: ctx.point_cloud_fovea(
        D.d["sx"], D.d["sy"], D.d["sc"], D.fw, D.fh, k, *D.maps[k], D.d["rgbF"], FW, FH, 3 * FW, D.P1, D.P2, prm, p, cap, c))
    return [got], [cn.cloud_fovea(lo, D.sx, D.sy, k, *D.maps[k], D.rgbF, D.P1, D.P2, stackc=D.sc, fmt=XYZ16)]


def case_fovea_all(compact):
    def case(ctx, lib, D, lo):
        kw = dict(min_conf=0.2, z_min=D.zwin_f[0], z_max=D.zwin_f[1]) if compact else {}
        prm = lib.cloud_params(format=PCL32, compact=compact, **kw)
        d_lvl = ctx.to_device(np.full(FF, -7, np.int64))
        per = []
        try:
            def call(p, cap, c):
                n, lv = ctx.point_cloud_fovea_all(D.d["sx"], D.d["sy"], D.d["sc"], FW, FH, OFF, D.d["rgbF"], 3 * FW, D.P1, D.P2, prm, p, cap, c, d_lvl)
                per.extend(lv)
                return n
            got = _cloud_call(ctx, lib, PCL32, lib.fovea_cloud_points(FW, FH, FLV, FF, OFF, 1), call)
        finally:
            ctx.free(d_lvl)
        exp, exp_per = sn.cloud_fovea_all(lo, D.sx, D.sy, D.rgbF, OFF, D.P1, D.P2, stackc=D.sc, fmt=PCL32, compact=compact, **kw)
        assert sum(exp_per) < FF * D.fw * D.fh                  # (the window's finer levels cover part of the coarser ones)
        return [got, np.array(per, np.int64)], [exp, np.array(exp_per, np.int64)]
    return case


def case_resized(factor):
    def case(ctx, lib, D, lo):
        prm = lib.cloud_params(format=PCL32)
        got = _cloud_call(ctx, lib, PCL32, lib.resized_cloud_points(W, H, factor), lambda p, cap, c: ctx.point_cloud_resized(
            D.d["dxr"], D.d["dy"], D.d["conf"], D.d["rgb"], W, H, 3 * W, D.P1, D.P2, factor, prm, p, cap, c))
        if factor == 0.2:
            assert got.size == 19 * 26
        return [got], [rn.resized_cloud(lo, D.dxr, D.dy, D.rgb, D.P1, D.P2, factor, conf=D.conf, fmt=PCL32)]
    return case


def case_resized_fovea(ctx, lib, D, lo):
    k, factor = 1, 0.5
    prm = lib.cloud_params(format=XYZ16, compact=True, min_conf=0.2)
    got = _cloud_call(ctx, lib, XYZ16, lib.resized_cloud_points(D.fw, D.fh, factor), lambda p, cap, c: ctx.point_cloud_resized_fovea(
        D.d["sx"], D.d["sy"], D.d["sc"], D.fw, D.fh, k, *D.maps[k], D.d["rgbF"], FW, FH, 3 * FW, D.P1, D.P2, factor, prm, p, cap, c))
    return [got], [rn.resized_cloud_fovea(lo, D.sx, D.sy, k, *D.maps[k], D.rgbF, D.P1, D.P2, factor, stackc=D.sc, fmt=XYZ16, compact=True, min_conf=0.2)]


def _depth_kw(D, fmt, fovea=False):
    win = D.zwin_f if fovea else D.zwin
    return dict(fmt=dn.FMT_16U, unit=D.unit, min_conf=0.15) if fmt == dn.FMT_16U else dict(fmt=dn.FMT_32F, unit=0.25, z_min=win[0], z_max=win[1], min_conf=0.1)


def case_depth(fmt, factor):
    def case(ctx, lib, D, lo):
        kw = _depth_kw(D, fmt)
        prm = lib.depth_params(format=fmt, factor=factor, **{k: v for k, v in kw.items() if k != "fmt"})
        dx = D.d["dx"] if factor == 1.0 else D.d["dxr"]
        img, counts = _depth_call(ctx, lib, prm, W, H, 1, lambda o, v: ctx.depth_image(dx, D.d["dy"], D.d["conf"], W, H, D.P1, D.P2, prm, o, v))
        exp, valid = dn.depth_image(lo, D.dx if factor == 1.0 else D.dxr, D.dy, D.P1, D.P2, conf=D.conf, factor=factor, **kw)
        assert 0.05 < valid.mean() < 0.95                       # (both branches)
        return [img[0], counts], [exp, np.array([int(valid.sum())], np.int64)]
    return case


def case_depth_fovea(ctx, lib, D, lo):
    kw = _depth_kw(D, dn.FMT_32F, fovea=True)
    prm = lib.depth_params(format=dn.FMT_32F, **{k: v for k, v in kw.items() if k != "fmt"})
    img, counts = _depth_call(ctx, lib, prm, D.fw, D.fh, FF, lambda o, v: ctx.depth_image_fovea(
        D.d["sx"], D.d["sy"], D.d["sc"], FW, FH, OFF, lib.UGSM_DEPTH_ALL_LEVELS, D.P1, D.P2, prm, o, v))
    exp = [dn.depth_image_fovea(lo, D.sx, D.sy, k, *D.maps[k], D.P1, D.P2, stackc=D.sc, **kw) for k in range(FF)]
    return [img, counts], [np.stack([e for e, _ in exp]), np.array([int(v.sum()) for _, v in exp], np.int64)]


CASES = {
    "triangulate": case_tri, "triangulate_fovea level 0": case_tri_fovea(0), "triangulate_fovea level 2": case_tri_fovea(2),
    "point_cloud PCL32 s1": case_cloud(PCL32, 1, False), "point_cloud PCL32 s3": case_cloud(PCL32, 3, False),
    "point_cloud XYZRGB16 s1": case_cloud(XYZ16, 1, False), "point_cloud XYZRGB16 s3": case_cloud(XYZ16, 3, False),
    "point_cloud compact": case_cloud(PCL32, 1, True), "point_cloud_fovea level 1": case_cloud_fovea,
    "point_cloud_fovea_all dense": case_fovea_all(False), "point_cloud_fovea_all compact": case_fovea_all(True),
    "point_cloud_resized 0.2": case_resized(0.2), "point_cloud_resized 1": case_resized(1.0), "point_cloud_resized_fovea 0.5": case_resized_fovea,
    "depth_image 32F 1": case_depth(dn.FMT_32F, 1.0), "depth_image 32F 0.5": case_depth(dn.FMT_32F, 0.5),
    "depth_image 16U 1": case_depth(dn.FMT_16U, 1.0), "depth_image 16U 0.5": case_depth(dn.FMT_16U, 0.5),
    "depth_image_fovea all levels": case_depth_fovea,
}


def assert_same(got, exp, what):
    """Records byte for byte with a NaN X, Y or Z equal to any NaN; float planes the same way; images and counts exactly."""
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if g.dtype.names:
            cn.assert_cloud_equal(g, e, what)
        elif g.dtype == F32 and g.ndim == 3 and g.shape[0] == 3 and "depth" not in what:
            assert g.shape == e.shape
            same = (g.view(np.uint32) == np.ascontiguousarray(e, F32).view(np.uint32)) | (np.isnan(g) & np.isnan(e))
            assert same.all(), f"{what}: {int((~same).sum())} of {g.size} values differ"
        elif g.dtype == F32 or g.dtype == np.uint16:
            dn.assert_image_equal(g, e, what)
        else:
            assert np.array_equal(g, e), f"{what}: {g.tolist()} vs {e.tolist()}"


def zero_lens(rig, iterations=5):
    return rig["K1"], np.zeros(5), rig["K2"], np.zeros(5), iterations


@pytest.mark.parametrize("name", list(CASES))
def test_honoured_call_is_the_restatement_under_a_lens(lib, ctx, data, name):
    """7. With the small rig set, the device output of each honoured call equals lens_np bit for bit."""
    lens = ln.lens_of(data.rig)
    ctx.set_lens(*lens)
    try:
        got, exp = CASES[name](ctx, lib, data, ln.LensOracle(lens))
    finally:
        ctx.clear_lens()
    assert_same(got, exp, name)


@pytest.mark.parametrize("name", list(CASES))
def test_zero_distortion_and_a_cleared_lens_give_the_bytes_of_no_lens(lib, ctx, data, name):
    """8. / 9. The call with a zero-D lens set gives the call without a lens (a NaN X, Y or Z equal to any NaN: a NaN or infinite right
    position comes out of the undistortion as NaN in both coordinates), after ugsm_set_lens(NULL ...) again -- and the call without a lens is
    the restatement without one, while under the small rig some Z differ: the setting is not silently ignored."""
    assert ctx.get_lens() is None
    plain, exp = CASES[name](ctx, lib, data, ln.LensOracle(None))
    assert_same(plain, exp, name + " without a lens")
    ctx.set_lens(*zero_lens(data.rig))
    try:
        zero, _ = CASES[name](ctx, lib, data, ln.LensOracle(None))
        ctx.set_lens(*ln.lens_of(data.rig))
        bent, _ = CASES[name](ctx, lib, data, ln.LensOracle(None))
    finally:
        ctx.clear_lens()
    cleared, _ = CASES[name](ctx, lib, data, ln.LensOracle(None))
    assert_same(zero, plain, name + " with a zero-D lens")
    assert_same(cleared, plain, name + " after the lens was cleared")
    assert cleared[0].tobytes() == plain[0].tobytes()
    assert bent[0].shape != plain[0].shape or bent[0].tobytes() != plain[0].tobytes(), name + ": the lens changed nothing"


def test_match_full_depth_honours_the_lens(lib):
    """7., the blocking call on a 64 x 48 synthetic pair: the depth image equals the restatement applied to the planes the call returned, with
    the lens and with a zero-D lens (the bytes of no lens)."""
    from ug_stereomatcher_amd import synth
    rig = ln.rigs()["small"]
    L, R, _, _ = synth.make_pair(64, 48, synth.BASE_SEED + 7)
    prm = lib.depth_params(format=lib.UGSM_DEPTH_32F, unit=0.5)
    with lib.Context(levels=5) as c:
        plain, planes0 = c.match_full_depth(L, R, rig["P1"], rig["P2"], prm, planes=True)
        c.set_lens(*ln.lens_of(rig))
        bent, planes = c.match_full_depth(L, R, rig["P1"], rig["P2"], prm, planes=True)
        c.set_lens(*zero_lens(rig))
        zero, _ = c.match_full_depth(L, R, rig["P1"], rig["P2"], prm, planes=True)
    assert planes.tobytes() == planes0.tobytes()                # (the match does not see the lens)
    for img, lens, what in ((bent, ln.lens_of(rig), "lens"), (plain, None, "no lens")):
        z = ln.triangulate(planes[0], planes[1], rig["P1"], rig["P2"], lens)[2]
        exp, valid = dn.depth_of_z(z, conf=planes[2], fmt=dn.FMT_32F, unit=0.5)
        assert valid.mean() > 0.5
        dn.assert_image_equal(img, exp, "ugsm_match_full_depth, " + what)
    assert zero.tobytes() == plain.tobytes() and bent.tobytes() != plain.tobytes()


def test_a_call_captures_the_lens_it_was_made_under(lib, ctx, data):
    """10. On one slot: rig A set and a call, rig B set and a call into a second buffer, one wait -- the first buffer holds A's result, the
    second B's."""
    big = ln.rigs()["rig16mp"]
    A, B = ln.lens_of(data.rig), (big["K1"], big["D1"], big["K2"], big["D2"], 7)
    p1, p2, q1, q2 = ctx._proj(data.P1, data.P2)
    bufs = [_poisoned(ctx, 3 * W * H * 4) for _ in range(2)]
    try:
        for lens, out in ((A, bufs[0]), (B, bufs[1])):
            ctx.set_lens(*lens)
            ctx.check(ctx.lib.ugsm_triangulate(ctx.handle, 0, data.d["dx"], data.d["dy"], W, H, q1, q2, out))
        ctx.clear_lens()
        ctx.check(ctx.lib.ugsm_wait(ctx.handle, 0))
        got = [ctx.to_host(b, (3, H, W)) for b in bufs]
    finally:
        ctx.clear_lens()
        for b in bufs:
            ctx.free(b)
    expA, expB = (ln.triangulate(data.dx, data.dy, data.P1, data.P2, lens) for lens in (A, B))
    assert_same([got[0]], [expA], "the call made under rig A")
    assert_same([got[1]], [expB], "the call made under rig B")
    assert got[0].tobytes() != got[1].tobytes()


def test_refusals(lib, ctx, data):
    """11. With a lens set ugsm_point_cloud_fovea_multi and ugsm_enqueue_full_cloud answer UGSM_ERR_STATE, name the setting, write nothing and
    enqueue nothing; ugsm_set_lens refuses bad arguments and leaves the setting as it was."""
    so, h, STATE, BAD = ctx.lib, ctx.handle, lib.UGSM_ERR_STATE, lib.UGSM_ERR_BAD_ARG
    rig = data.rig
    dbl = lambda a: (C.c_double * np.size(a))(*np.asarray(a, np.float64).reshape(-1))      # noqa: E731
    K1, D1, K2, D2 = (dbl(rig[k]) for k in ("K1", "D1", "K2", "D2"))
    ctx.set_lens(*ln.lens_of(rig, 9))

    def setting():
        g = ctx.get_lens()
        return None if g is None else b"".join(np.asarray(v).tobytes() for v in g[:4]) + bytes([g[4]])
    before = setting()
    assert before is not None and ctx.get_lens()[4] == 9 and np.array_equal(ctx.get_lens()[0], rig["K1"]) and np.array_equal(ctx.get_lens()[3], rig["D2"])
    try:
        bad = lambda k, v: dbl(list(np.asarray(rig["K1"]).reshape(-1)[:k]) + [v] + list(np.asarray(rig["K1"]).reshape(-1)[k + 1:]))   # noqa: E731
        for args in ((K1, D1, K2, None, 5), (None, D1, K2, D2, 5), (K1, None, None, None, 5), (bad(2, np.nan), D1, K2, D2, 5),
                     (K1, dbl([np.inf, 0, 0, 0, 0]), K2, D2, 5), (K1, D1, K2, dbl([0, 0, 0, 0, -np.inf]), 5), (bad(0, 0.0), D1, K2, D2, 5),
                     (bad(0, -3.0), D1, K2, D2, 5), (K1, D1, bad(4, 0.0), D2, 5), (K1, D1, K2, D2, 33), (K1, D1, K2, D2, -1)):
            assert so.ugsm_set_lens(h, *args) == BAD, args[4]
            assert setting() == before
        assert b"ugsm_set_lens" in so.ugsm_last_error(h)
        # the merged cloud of several windows
        stack = np.concatenate([data.sx, data.sy, data.sc]).astype(F32)
        d_stack = ctx.to_device(stack)
        cap = lib.fovea_multi_cloud_points(FW, FH, FLV, FF, [OFF], 1)
        d_pts, d_cnt = _poisoned(ctx, cap * 32), _poisoned(ctx, 8)
        d_out, d_img = _poisoned(ctx, 3 * FW * FH * 4), ctx.to_device(data.rgbF)
        prm = lib.cloud_params()
        try:
            with pytest.raises(lib.UgsmError) as e:
                ctx.point_cloud_fovea_multi([d_stack], FW, FH, [OFF], data.d["rgbF"], 3 * FW, data.P1, data.P2, prm, d_pts, cap, d_cnt)
            assert e.value.status == STATE and "ugsm_set_lens" in str(e.value)
            spec = lib.queue_cloud(data.P1, data.P2, prm)
            with pytest.raises(lib.UgsmError) as e:
                ctx.enqueue_full_cloud(data.d["rgbF"], d_img, FW, FH, 3 * FW, d_out, spec, d_pts, cap, d_cnt, 1)
            assert e.value.status == STATE and "ugsm_set_lens" in str(e.value)
            assert ctx.queue_depth() == (0, 0, 0)
            ctx.check(so.ugsm_wait(h, 0))
            for p, n in ((d_pts, cap * 32), (d_cnt, 8), (d_out, 3 * FW * FH * 4)):
                assert (ctx.to_host(p, (n,), np.uint8) == POISON).all(), "a refused call wrote to its output"
            ctx.clear_lens()                                     # ... and both are served again without a lens
            assert ctx.point_cloud_fovea_multi([d_stack], FW, FH, [OFF], data.d["rgbF"], 3 * FW, data.P1, data.P2, prm, d_pts, cap, d_cnt) == cap
        finally:
            for p in (d_stack, d_pts, d_cnt, d_out, d_img):
                ctx.free(p)
    finally:
        ctx.clear_lens()
    assert ctx.get_lens() is None


def test_input_format_changes_only_the_colour_word_under_a_lens(lib, ctx, data):
    """12. A bgr8 image and a mono32f image give the X, Y, Z of the rgb8 call under a lens; only the colour word differs, as without one."""
    lens = ln.lens_of(data.rig)
    prm = lib.cloud_params(format=XYZ16)
    mono = data.rgb[..., 1].astype(F32)
    images = {lib.UGSM_INPUT_RGB8: (data.rgb, 3 * W, cn.colour_word(data.rgb)),
              lib.UGSM_INPUT_BGR8: (np.ascontiguousarray(data.rgb[..., ::-1]), 3 * W, cn.colour_word(data.rgb)),
              lib.UGSM_INPUT_MONO32F: (mono, 4 * W, data.rgb[..., 1].astype(np.uint32) * 0x010101)}
    xyz = ln.triangulate(data.dx, data.dy, data.P1, data.P2, lens)
    ctx.set_lens(*lens)
    try:
        for fmt, (img, stride, word) in images.items():
            ctx.set_input_format(fmt)
            d_img = ctx.to_device(img)
            try:
                got = _cloud_call(ctx, lib, XYZ16, W * H, lambda p, cap, c: ctx.point_cloud(
                    data.d["dx"], data.d["dy"], None, d_img, W, H, stride, data.P1, data.P2, prm, p, cap, c))
            finally:
                ctx.free(d_img)
            cn.assert_cloud_equal(got, cn.records(xyz, word, fmt=XYZ16), f"input format {fmt}")
    finally:
        ctx.set_input_format(lib.UGSM_INPUT_RGB8)
        ctx.clear_lens()
