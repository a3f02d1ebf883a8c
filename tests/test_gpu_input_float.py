"""The float input formats (UGSM_INPUT_RGB32F, UGSM_INPUT_MONO32F) on the device.  Every comparison is on bit patterns.

1. A float image whose samples are the integers 0 .. 255 gives, byte for byte, the rgb8 (mono8) call's result on those bytes, for every
   entry point that takes an image: 157 x 101 with packed and padded rows, and 160 x 104 (the 16-byte store paths) with the images at + 4,
   + 8 and + 12 bytes of an allocation.
2. Fractional samples (a 16-bit-like image / 256): the full-mode call equals the CPU oracle's stages started from the float planes
   (tests/float_np.py cold_float), the L / R pyramid stacks of a foveated call equal the crops of orc.pyramid, ugsm_stage_pyramid equals it.
3. The range word: a float level 0 is the caller's, so the pyramid kernels check the samples they load.
4. The alignment and stride refusals, the format left as it was.
5. ugsm_set_input_format(8) and (9) succeed.
"""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import dark_np as dk
import encode_np as en
import float_np as fl
from conftest import assert_bit_equal
from test_gpu_cloud import P1, P2A

pytestmark = pytest.mark.gpu

W, H, LEVELS, F = 157, 101, 8, 4
W4, H4 = 160, 104  # a width that is a multiple of 4: level 0 leaves as 16-byte stores
PAD = 8
IDS = [fl.NAMES[f] for f in fl.FORMATS]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def _pair(w, h, seed):
    from ug_stereomatcher_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    L, R, _, _ = synth.make_pair(w, h, synth.BASE_SEED + seed)
    L.reshape(-1, 3)[rng.integers(0, w * h, 200)] = (255, 0, 17)  # saturated and zero samples: a channel mix-up cannot hide
    return L, R


@pytest.fixture(scope="module")
def pair():
    return _pair(W, H, 61)


@pytest.fixture(scope="module")
def pair2():
    return _pair(W, H, 62)


@pytest.fixture(scope="module")
def pair4():
    return _pair(W4, H4, 63)


@pytest.fixture(scope="module")
def ctx(lib):
    with lib.Context(levels=LEVELS, fovea_levels=F, slots=2, batch=3) as c:
        yield c


def _eight(L, R, fmt):
    """The 8-bit pair an integer-valued float pair in `fmt` must agree with, and its format."""
    e = fl.EIGHT_BIT[fmt]
    return (en.encode(L, e), en.encode(R, e)), e


def _float(L, R, fmt):
    return fl.encode(L, fmt), fl.encode(R, fmt)


class Dev:
    """Device copies of images of any format: rows padded by `pad` bytes, the first byte at `shift` past an allocation."""

    def __init__(self, c):
        self.c, self.bufs = c, []

    def put(self, img, pad=0, shift=0):
        rows = fl.rows(img, pad)
        base = self.c.alloc(rows.nbytes + 64)
        self.bufs.append(base)
        raw = np.full(rows.nbytes + 64, 0xA5, np.uint8)
        raw[shift:shift + rows.nbytes] = rows.reshape(-1)
        self.c.check(self.c.lib.ugsm_copy_to_device(self.c.handle, base, raw.ctypes.data, raw.nbytes))
        return base + shift, rows.shape[1]

    def floats(self, a):
        p = self.c.to_device(np.ascontiguousarray(a, np.float32))
        self.bufs.append(p)
        return p

    def out(self, nfloats):
        p = self.c.alloc(4 * nfloats + 64)
        self.bufs.append(p)
        self.c.check(self.c.lib.ugsm_copy_to_device(self.c.handle, p, np.full(nfloats, np.nan, np.float32).ctypes.data, 4 * nfloats))
        return p

    def free(self):
        for p in self.bufs:
            self.c.free(p)
        self.bufs = []


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _full(c, fmt, imgs, pad=0, shift=0, slot=0):
    h, w = imgs[0].shape[:2]
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        (pl, stride), (pr, _) = d.put(imgs[0], pad, shift), d.put(imgs[1], pad, shift)
        o = d.out(3 * w * h)
        c.check(c.lib.ugsm_submit_full(c.handle, slot, pl, pr, w, h, stride, o))
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return c.to_host(o, (3, h, w))
    finally:
        d.free()
        c.set_input_format(en.RGB8)


def _foveated(c, lib, fmt, imgs, off, pad=0, shift=0):
    """(stack, pyrL, pyrR) of ugsm_submit_foveated, each flat."""
    h, w = imgs[0].shape[:2]
    fw, fh = (int(v) for v in lib.fovea_dims(w, h, LEVELS, F))
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        (pl, stride), (pr, _) = d.put(imgs[0], pad, shift), d.put(imgs[1], pad, shift)
        o, yl, yr = d.out(3 * F * fh * fw), d.out(3 * F * fh * fw), d.out(3 * F * fh * fw)
        c.check(c.lib.ugsm_submit_foveated(c.handle, 0, pl, pr, w, h, stride, off[0], off[1], o, yl, yr))
        c.check(c.lib.ugsm_wait(c.handle, 0))
        return [c.to_host(p, (3 * F * fh * fw,)) for p in (o, yl, yr)]
    finally:
        d.free()
        c.set_input_format(en.RGB8)


# ---- 5. the setter ---------------------------------------------------------------------------------------------------------------------

def test_the_setter_takes_the_two_formats(lib, ctx):
    for f in fl.FORMATS:
        ctx.set_input_format(f)
        assert ctx.input_format == f
    for bad in (5, 6, 7, 10, 99):
        with pytest.raises(lib.UgsmError) as e:
            ctx.set_input_format(bad)
        assert e.value.status == lib.UGSM_ERR_BAD_ARG and ctx.input_format == fl.MONO32F
    ctx.set_input_format(en.RGB8)


# ---- 1. integer-valued float images against the 8-bit call -----------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_full_and_foveated_calls_equal_the_8bit_call(lib, ctx, pair, fmt):
    """k_pyr_base (full calls) and k_pyr_base_march (foveated calls: the stack and both pyramid stacks, off-centre window); packed and padded rows."""
    eight, e = _eight(*pair, fmt)
    imgs = _float(*pair, fmt)
    want_full = _full(ctx, e, eight)
    want_fov = _foveated(ctx, lib, e, eight, (5, -3))
    for pad in (0, PAD):
        assert np.array_equal(_bits(_full(ctx, fmt, imgs, pad)), _bits(want_full)), pad
        for g, w, what in zip(_foveated(ctx, lib, fmt, imgs, (5, -3), pad), want_fov, ("stack", "pyrL", "pyrR")):
            assert np.array_equal(_bits(g), _bits(w)), (what, pad)


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_width_multiple_of_4_at_every_4_byte_base(lib, ctx, pair4, fmt):
    """160 x 104: level 0 leaves as 16-byte stores; the images at + 4, + 8 and + 12 bytes of an allocation (a float image needs 4-byte
    alignment and no more)."""
    eight, e = _eight(*pair4, fmt)
    imgs = _float(*pair4, fmt)
    want_full = _full(ctx, e, eight)
    want_fov = _foveated(ctx, lib, e, eight, (-4, 2))
    for pad, shift in ((0, 4), (PAD, 8), (0, 12), (4, 0)):
        assert np.array_equal(_bits(_full(ctx, fmt, imgs, pad, shift)), _bits(want_full)), (pad, shift)
        for g, w, what in zip(_foveated(ctx, lib, fmt, imgs, (-4, 2), pad, shift), want_fov, ("stack", "pyrL", "pyrR")):
            assert np.array_equal(_bits(g), _bits(w)), (what, pad, shift)


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_two_level_pyramids_read_the_format(lib, pair, fmt):
    """levels = 2: no k_pyr_base; level 0 comes from k_rgb_planes."""
    eight, e = _eight(*pair, fmt)
    imgs = _float(*pair, fmt)
    with lib.Context(levels=2, fovea_levels=2) as c:
        want = _full(c, e, eight)
        for pad in (0, PAD):
            assert np.array_equal(_bits(_full(c, fmt, imgs, pad)), _bits(want)), pad


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_batch_host_managed_queue_and_service_calls(lib, ctx, pair, pair2, fmt):
    c = ctx
    eight0, e8 = _eight(*pair, fmt)
    eight1 = _eight(*pair2, fmt)[0]
    a, b = _float(*pair, fmt)
    a2, b2 = _float(*pair2, fmt)
    want = [_full(c, e8, eight0), _full(c, e8, eight1)]
    rgb_want = _full(c, en.RGB8, pair)
    # ugsm_submit_full_batch: two pairs, one launch per level for both, the second pair's images 4 bytes further on in their allocations
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        (l0, stride), (r0, _) = d.put(a, PAD), d.put(b, PAD)
        (l1, _), (r1, _) = d.put(a2, PAD, 4), d.put(b2, PAD, 4)
        outs = [d.out(3 * W * H), d.out(3 * W * H)]
        c.submit_full_batch(0, [l0, l1], [r0, r1], W, H, stride, outs)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        for k in range(2):
            assert np.array_equal(_bits(c.to_host(outs[k], (3, H, W))), _bits(want[k])), ("batch", k)
        # the device queue: an rgb8 pair between two float pairs -- pairs of different formats never share a call
        q = [d.out(3 * W * H) for _ in range(3)]
        pl8, s8 = d.put(pair[0])
        pr8, _ = d.put(pair[1])
        c.enqueue_full(l0, r0, W, H, stride, q[0], 0)
        c.set_input_format(en.RGB8)
        c.enqueue_full(pl8, pr8, W, H, s8, q[1], 1)
        c.set_input_format(fmt)
        c.enqueue_full(l1, r1, W, H, stride, q[2], 2)
        done = c.drain()
        assert [x.tag for x in done] == [0, 1, 2]
        assert len({int(x.call_index) for x in done}) == 3
        for k, w in enumerate((want[0], rgb_want, want[1])):
            assert np.array_equal(_bits(c.to_host(q[k], (3, H, W))), _bits(w)), ("device queue", k)
    finally:
        d.free()
    # page-locked host memory: ugsm_submit_full_host
    hl, hr = c.host_array(a.shape, np.float32), c.host_array(b.shape, np.float32)
    hl[...], hr[...] = a, b
    hout = c.host_array((3, H, W), np.float32)
    c.check(c.lib.ugsm_submit_full_host(c.handle, 1, hl.ctypes.data, hr.ctypes.data, W, H, hl.strides[0], hout[0].ctypes.data,
                                        hout[1].ctypes.data, hout[2].ctypes.data))
    c.check(c.lib.ugsm_wait(c.handle, 1))
    assert np.array_equal(_bits(hout), _bits(want[0])), "_host"
    # ... and through the queue
    hout[...] = np.nan
    c.enqueue_full_host(hl, hr, hout, 7)
    assert [x.tag for x in c.drain()] == [7]
    assert np.array_equal(_bits(hout), _bits(want[0])), "queue, _host"
    # the service call from pageable memory, padded rows (ugsm_match_full)
    rowsL, rowsR = fl.rows(a, PAD), fl.rows(b, PAD)
    out = np.full((3, H, W), np.nan, np.float32)
    c.check(c.lib.ugsm_match_full(c.handle, rowsL.ctypes.data, rowsR.ctypes.data, W, H, rowsL.shape[1], out[0].ctypes.data, out[1].ctypes.data,
                                  out[2].ctypes.data))
    assert np.array_equal(_bits(out), _bits(want[0])), "ugsm_match_full"
    # managed queue calls, an rgb8 pair between the two float pairs; the first with padded input rows
    pa = fl.rows(a, PAD)[:, :a[0].nbytes].view(np.float32).reshape(a.shape)
    pb = fl.rows(b, PAD)[:, :b[0].nbytes].view(np.float32).reshape(b.shape)
    assert pa.strides[0] == a.strides[0] + PAD
    c.enqueue_full_managed(pa, pb, 1)
    c.set_input_format(en.RGB8)
    c.enqueue_full_managed(pair[0], pair[1], 2)
    c.set_input_format(fmt)
    c.enqueue_full_managed(a2, b2, 3)
    for k, w in enumerate((want[0], rgb_want, want[1])):
        done = c.next_done(True)
        assert done.tag == k + 1
        planes = np.stack(c.managed_planes(done, [(H, W)] * 3))
        assert np.array_equal(_bits(planes), _bits(w)), ("managed", k)
    # the NumPy-taking methods check dtype and shape against the format
    wrong = np.zeros((H, W, 3), np.uint8)
    with pytest.raises(lib.UgsmError):
        c.enqueue_full_managed(wrong, wrong, 0)
    c.set_input_format(en.RGB8)


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_multi_window_call_reads_level_0_inside_the_windows(lib, ctx, pair, fmt):
    """ugsm_submit_foveated_multi with two windows: k_pyr_base stores no level 0, k_level0_windows converts it inside the windows."""
    c = ctx
    fw, fh = (int(v) for v in lib.fovea_dims(W, H, LEVELS, F))
    offs = [(9, -6), (-14, 4)]

    def run(f, imgs, pad):
        c.set_input_format(f)
        d = Dev(c)
        try:
            (pl, stride), (pr, _) = d.put(imgs[0], pad), d.put(imgs[1], pad)
            stacks = [d.out(3 * F * fh * fw) for _ in offs]
            c.submit_foveated_multi(0, pl, pr, W, H, stride, offs, stacks)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            return [c.to_host(s, (3 * F * fh * fw,)) for s in stacks]
        finally:
            d.free()
            c.set_input_format(en.RGB8)

    eight, e = _eight(*pair, fmt)
    want = run(e, eight, 0)
    for pad in (0, PAD):
        for k, (g, w) in enumerate(zip(run(fmt, _float(*pair, fmt), pad), want)):
            assert np.array_equal(_bits(g), _bits(w)), (pad, k)


def _clouds(c, lib, fmt, img, planes, stack, compact, pad, off):
    """ugsm_point_cloud and ugsm_point_cloud_fovea_all coloured from `img` in `fmt`: (count, record bytes) of each."""
    c.set_input_format(fmt)
    d = Dev(c)
    res = []
    try:
        p_img, stride = d.put(img, pad)
        dx, dy, cf = (d.floats(a) for a in planes)
        sx, sy, sc = (d.floats(a) for a in stack)
        params = lib.cloud_params(format=cn.PCL32, compact=compact, min_conf=0.2 if compact else None)
        for kind in ("dense", "fovea_all"):
            cap = W * H if kind == "dense" else lib.fovea_cloud_points(W, H, LEVELS, F, off)
            pts = d.out(8 * (cap + 16))
            cnt = c.to_device(np.full(1, -7, np.int64))
            d.bufs.append(cnt)
            if kind == "dense":
                n = c.point_cloud(dx, dy, cf, p_img, W, H, stride, P1, P2A, params, pts, cap, cnt)
            else:
                n = c.point_cloud_fovea_all(sx, sy, sc, W, H, off, p_img, stride, P1, P2A, params, pts, cap, cnt)
            res.append((n, c.to_host(pts, (min(n, cap) * 32,), np.uint8)))
    finally:
        d.free()
        c.set_input_format(en.RGB8)
    return res


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_cloud_calls_colour_from_a_float_image(lib, ctx, pair, fmt):
    rng = np.random.Generator(np.random.PCG64(99 + fmt))
    fw, fh = (int(v) for v in lib.fovea_dims(W, H, LEVELS, F))
    planes = (rng.normal(-40, 25, (H, W)).astype(np.float32), rng.normal(0, 2, (H, W)).astype(np.float32),
              rng.uniform(0, 1, (H, W)).astype(np.float32))
    stack = (rng.normal(-20, 9, (F * fh, fw)).astype(np.float32), rng.normal(0, 1, (F * fh, fw)).astype(np.float32),
             rng.uniform(0, 1, (F * fh, fw)).astype(np.float32))
    e = fl.EIGHT_BIT[fmt]
    img8 = en.encode(pair[0], e)
    img = fl.encode(pair[0], fmt)
    for compact in (False, True):
        got = _clouds(ctx, lib, fmt, img, planes, stack, compact, PAD, (5, -3))
        want = _clouds(ctx, lib, e, img8, planes, stack, compact, PAD, (5, -3))
        for k, ((n, g), (m, w)) in enumerate(zip(got, want)):
            assert n == m and n > 0 and np.array_equal(g, w), (k, compact)
    # the colour word's rule on samples that are no integers: fractions either side of .5, values past both ends, a NaN
    frac = img.copy()
    flat = frac.reshape(-1)
    flat[:] = flat + rng.uniform(-0.75, 0.75, flat.size).astype(np.float32)
    flat[rng.integers(0, flat.size, 50)] = np.float32(300.0)
    flat[rng.integers(0, flat.size, 50)] = np.float32(-2.0)
    flat[rng.integers(0, flat.size, 50)] = np.float32(np.nan)
    flat[:4] = np.array([0.49, 0.5, 254.5, 254.49], np.float32)
    n, raw = _clouds(ctx, lib, fmt, frac, planes, stack, False, 0, (0, 0))[0]
    words = raw.view(cn.DTYPES[cn.PCL32])["rgb"]
    assert n == W * H and np.array_equal(words, cn.column_major(fl.colour_word(frac, fmt), 1))


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_warp_right_and_photometric_residual(lib, ctx, pair, fmt):
    c = ctx
    rng = np.random.Generator(np.random.PCG64(7 + fmt))
    dxy = (rng.normal(-6, 4, (H, W)).astype(np.float32), rng.normal(0, 1.5, (H, W)).astype(np.float32))
    conf = rng.uniform(0, 1, (H, W)).astype(np.float32)

    def run(f, imgs, pad):
        c.set_input_format(f)
        d = Dev(c)
        try:
            (pl, stride), (pr, _) = d.put(imgs[0], pad), d.put(imgs[1], pad)
            dx, dy, cf = d.floats(dxy[0]), d.floats(dxy[1]), d.floats(conf)
            o = d.out(3 * W * H)
            c.warp_right(pr, W, H, stride, dx, dy, o)
            warp = c.to_host(o, (3, H, W))
            c.photometric_residual(pl, pr, W, H, stride, dx, dy, cf)
            return warp, c.last_residual_sums.copy()
        finally:
            d.free()
            c.set_input_format(en.RGB8)

    eight, e = _eight(*pair, fmt)
    want_warp, want_sums = run(e, eight, 0)
    assert np.isfinite(want_sums).all() and want_sums[0, 3] > 0
    for pad in (0, PAD):
        warp, sums = run(fmt, _float(*pair, fmt), pad)
        assert np.array_equal(_bits(warp), _bits(want_warp)), pad
        assert np.array_equal(sums.view(np.uint64), want_sums.view(np.uint64)), pad


def test_python_class_and_service_take_float_arrays_in_place(lib, pair):
    """MatchGPULib.match on float32 (H, W, 3) and (H, W) arrays, a uint8 call in between (the format follows the array), and the service on
    32FC3 / 32FC1 messages with padded rows."""
    from ug_stereomatcher_amd import service as svc
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    m = MatchGPULib(levels=LEVELS)
    try:
        for fmt in fl.FORMATS:
            a, b = _float(*pair, fmt)
            eight = tuple(np.ascontiguousarray(fl.planes(i, fmt).transpose(1, 2, 0).astype(np.uint8)) for i in (a, b))  # rgb8 of (v, v, v) for mono
            want = m.match(eight[0], eight[1])
            assert np.array_equal(_bits(m.match(a, b)), _bits(want)), fl.NAMES[fmt]
            node = svc.GPUMatcher(matcher=m)
            msgs = []
            for img in (a, b):
                rows = fl.rows(img, PAD)
                msgs.append(svc.Image(svc.Header(), H, W, fl.ENCODINGS[fmt], 0, rows.shape[1], rows.tobytes()))
            rsp = svc.GetDisparitiesGPUResponse()
            assert node.disparitySrv(svc.GetDisparitiesGPURequest(*msgs), rsp)
            got = np.stack([rsp.dispH.image.to_array(), rsp.dispV.image.to_array(), rsp.dispC.image.to_array()])
            assert np.array_equal(_bits(got), _bits(want)), ("service", fl.NAMES[fmt])
    finally:
        m.close()


# ---- 2. fractional samples against the oracle's stages ---------------------------------------------------------------------------------

def _sixteen_bit_like(img8):
    """An (H, W, 3) uint8 image as float samples with 16 significant bits: (256 v + ramp) / 256, in [0, 256) and no integers (ramp >= 1)."""
    h, w = img8.shape[:2]
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    ramp = 1 + (x * 7 + y * 13 + ch * 29) % 255
    v = (img8.astype(np.float64) * 256 + ramp) / 256
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v) and out.min() > 0 and out.max() < 256 and not (out == np.floor(out)).any()
    return out


@pytest.fixture(scope="module")
def frac(orc, pair):
    """Per format: the fractional pair as images and planes, the oracle's pyramids of the planes and the cold full-mode field."""
    out = {}
    for fmt in fl.FORMATS:
        imgs = tuple(fl.encode(_sixteen_bit_like(p), fmt) for p in pair)
        pl, pr = fl.planes(imgs[0], fmt), fl.planes(imgs[1], fmt)
        out[fmt] = dict(imgs=imgs, pyrL=orc.pyramid(pl, LEVELS), pyrR=orc.pyramid(pr, LEVELS), full=fl.cold_float(orc, pl, pr, LEVELS))
    return out


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_fractional_full_mode_equals_the_oracles_stages(lib, ctx, frac, fmt):
    f = frac[fmt]
    for pad, shift in ((0, 0), (PAD, 4)):
        assert_bit_equal(_full(ctx, fmt, f["imgs"], pad, shift), f["full"], f"{fl.NAMES[fmt]}, pad {pad}, shift {shift}")
    if fmt == fl.MONO32F:  # bit for bit RGB32F of (v, v, v)
        rgb = tuple(np.ascontiguousarray(np.repeat(i[..., None], 3, axis=2)) for i in f["imgs"])
        assert_bit_equal(_full(ctx, fl.RGB32F, rgb), f["full"], "rgb32f of (v, v, v)")


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_fractional_pyramid_stacks_are_crops_of_the_oracles_pyramid(lib, ctx, orc, frac, fmt):
    """The streaming k_pyr_base_march with real floats: the L / R pyramid stacks of ugsm_submit_foveated are the oracle's levels 0 .. F-2
    cropped at orc.fovea_geometry, and level F-1 whole."""
    f, off = frac[fmt], (5, -3)
    fw, fh, ox, oy, _, _ = orc.fovea_geometry(W, H, LEVELS, F, off[0], off[1])
    _, gl, gr = _foveated(ctx, lib, fmt, f["imgs"], off, PAD)
    for got, pyr, side in ((gl, f["pyrL"], "L"), (gr, f["pyrR"], "R")):
        got = got.reshape(F, 3, fh, fw)
        for k in range(F):
            want = pyr[k] if k == F - 1 else pyr[k][:, oy[k]:oy[k] + fh, ox[k]:ox[k] + fw]
            assert_bit_equal(got[k], want, f"{fl.NAMES[fmt]} pyr{side} level {k}")


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_fractional_stage_pyramid_equals_the_oracles(lib, ctx, orc, frac, fmt):
    c, f = ctx, frac[fmt]
    w, h = (list(v) for v in lib.level_dims(W, H, LEVELS))
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        p, stride = d.put(f["imgs"][0], PAD, 8)
        for level in (0, 1, 2, 3, LEVELS - 1):
            o = d.out(3 * w[level] * h[level])
            c.check(c.lib.ugsm_stage_pyramid(c.handle, p, W, H, stride, level, o))
            assert_bit_equal(c.to_host(o, (3, h[level], w[level])), f["pyrL"][level], f"{fl.NAMES[fmt]} level {level}")
    finally:
        d.free()
        c.set_input_format(en.RGB8)


# ---- 3. the range word -----------------------------------------------------------------------------------------------------------------

def _word(orc, pl, pr, first=0):
    """1 where a value of the levels first .. of either pyramid fails range_ok (csrc/ugsm_exact.hpp), and the per-level counts."""
    cl = [int((~dk.in_range(p)).sum()) for p in orc.pyramid(pl, LEVELS)]
    cr = [int((~dk.in_range(p)).sum()) for p in orc.pyramid(pr, LEVELS)]
    return int(sum(cl[first:]) + sum(cr[first:]) > 0), cl, cr


def _range_cases(pair):
    """name -> (L, R) as (H, W, 3) float32.  A level-0 sample outside range_ok: 2^-40 (below 2^-12), 60000 (above 2^9), 600 on a textured image
    (its blurred fringe at levels 1 and up stays inside: only the check of level 0 itself can see it)."""
    L, R = (p.astype(np.float32) for p in pair)
    black = np.zeros((H, W, 3), np.float32)
    tiny, big = np.float32(2.0 ** -40), np.float32(60000.0)
    cases = {}
    a = black.copy()
    a[H // 2, W // 2, 0] = tiny
    cases["a: black, one 2^-40"] = (a, black.copy())
    b = L.copy()
    b[H // 3, W // 3, 0] = big
    cases["b: one 60000"] = (b, R.copy())
    # x = 64: the first column of the second 64-wide tile, a halo column of the first; x = 1, y = 1: outside the fovea window
    c1, c2 = L.copy(), R.copy()
    c1[20, 64, 0] = tiny
    c2[1, 1, 0] = big
    cases["c: 2^-40 in a halo column, 60000 outside the window"] = (c1, c2)
    e = np.clip(L, 64, 200)
    e[H // 2 + 3, W // 2 - 5, 0] = np.float32(600.0)
    cases["e: one 600 on a bright image"] = (e, np.clip(R, 64, 200))
    cases["d: in range"] = (L.copy(), R.copy())
    return cases


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_range_word_of_float_level_0(lib, orc, pair, fmt):
    """A float level 0 is the caller's: k_pyr_base and k_pyr_base_march check every in-image sample they load, so the pair's word is set
    for (a) - (c) and (e) and clear for (d), and full mode equals cold_float either way.  Case (e) is the one that fails when level 0 goes
    unchecked (its premise: no out-of-range value at any level above 0).  Whether (a) makes the two division paths give different bits on
    hardware has not been checked: either way it is a parity case, and the word is what this test observes."""
    with lib.Context(levels=LEVELS, fovea_levels=F, slots=1, dev=True) as c:
        for name, (L, R) in _range_cases(pair).items():
            imgs = fl.encode(L, fmt), fl.encode(R, fmt)
            pl, pr = fl.planes(imgs[0], fmt), fl.planes(imgs[1], fmt)
            word, cl, cr = _word(orc, pl, pr)
            print(f"[range word] {fl.NAMES[fmt]} {name}: out-of-range values per level L {cl} R {cr} -> word {word}")
            assert word == (0 if name.startswith("d") else 1), name
            if name.startswith("e"):
                assert sum(cl[1:]) + sum(cr[1:]) == 0 and cl[0] >= 1, (cl, cr)
            got = _full(c, fmt, imgs)
            assert c.range_words(0, 1) == [word], name
            assert_bit_equal(got, fl.cold_float(orc, pl, pr, LEVELS), f"{fl.NAMES[fmt]} {name}")
            if name.startswith(("c", "e", "d")):  # the streaming form, level 0 stored inside the window alone: the word covers the whole image
                _foveated(c, lib, fmt, imgs, (0, 0))
                assert c.range_words(0, 1) == [word], (name, "foveated")


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_range_word_of_a_two_level_pyramid(lib, orc, pair, fmt):
    """levels = 2: level 0 comes from k_rgb_planes, and is scanned once written."""
    L, R = _range_cases(pair)["e: one 600 on a bright image"]
    with lib.Context(levels=2, fovea_levels=2, dev=True) as c:
        for imgs, word in (((L, R), 1), ((np.clip(L, 0, 255), R), 0)):
            imgs = fl.encode(imgs[0], fmt), fl.encode(imgs[1], fmt)
            got = _full(c, fmt, imgs)
            assert c.range_words(0, 1) == [word]
            assert_bit_equal(got, fl.cold_float(orc, fl.planes(imgs[0], fmt), fl.planes(imgs[1], fmt), 2), fl.NAMES[fmt])


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", fl.FORMATS, ids=IDS)
def test_refusals_leave_the_format_as_it_was(lib, ctx, pair, fmt):
    c = ctx
    bpp = fl.BPP[fmt]
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        p, stride = d.put(fl.encode(pair[0], fmt), 16)
        assert stride == bpp * W + 16 and p % 4 == 0
        o = d.out(3 * W * H)
        cases = [(p + 1, p, stride, lib.UGSM_ERR_BAD_ARG), (p + 2, p, stride, lib.UGSM_ERR_BAD_ARG), (p, p + 1, stride, lib.UGSM_ERR_BAD_ARG),
                 (p, p, bpp * W + 2, lib.UGSM_ERR_BAD_ARG), (p, p, bpp * W - 4, lib.UGSM_ERR_SIZE_MISMATCH)]
        host = np.zeros(H * stride + 8, np.uint8)
        hp = host.ctypes.data + (-host.ctypes.data % 4)
        res = np.zeros((3, H, W), np.float32)
        for l, r, s, want in cases:
            assert c.lib.ugsm_submit_full(c.handle, 0, l, r, W, H, s, o) == want, (l - p, r - p, s)
            assert c.lib.ugsm_enqueue_full(c.handle, l, r, W, H, s, o, 0) == want, (l - p, r - p, s)
            assert c.lib.ugsm_submit_foveated(c.handle, 0, l, r, W, H, s, 0, 0, o, None, None) == want, (l - p, r - p, s)
            if l == p:
                assert c.lib.ugsm_stage_pyramid(c.handle, r, W, H, s, 0, o) == want, (r - p, s)
            assert c.lib.ugsm_match_full(c.handle, hp + (l - p), hp + (r - p), W, H, s, res[0].ctypes.data, res[1].ctypes.data,
                                         res[2].ctypes.data) == want, (l - p, r - p, s)
            assert c.input_format == fmt
        # the warp and the clouds answer UGSM_ERR_BAD_ARG for every one of them, as they do for rgb8
        for l, r, s, _ in cases:
            if l == p:
                assert c.lib.ugsm_warp_right(c.handle, 0, r, W, H, s, o, o, o) == lib.UGSM_ERR_BAD_ARG
        assert c.queue_depth() == (0, 0, 0)
        assert c.lib.ugsm_wait(c.handle, 0) == lib.UGSM_OK
        # nothing was enqueued and nothing stuck: the aligned call still runs
        c.check(c.lib.ugsm_submit_full(c.handle, 0, p, p, W, H, stride, o))
        c.check(c.lib.ugsm_wait(c.handle, 0))
    finally:
        d.free()
        c.set_input_format(en.RGB8)
