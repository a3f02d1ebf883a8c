"""The input formats (ugsm_set_input_format, UGSM_INPUT_*) on the device: a call on an image in format F gives, byte for byte, the rgb8 call's
result on the image's conversion to rgb8 (tests/encode_np.py) -- full, foveated with the L / R pyramid stacks, batched, page-locked (_host),
managed and device-queue calls, the pageable service call, the pyramids of fewer than three levels (k_rgb_planes), the four cloud calls and the
fovea shard; and the formats against the CPU oracle.  Widths that are no multiple of 4, padded strides and a 1-byte misaligned four-byte
image (the byte-load forms) next to aligned ones (the word-load forms)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cloud_np as cn
import encode_np as en
from test_gpu_cloud import P1, P2A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS, F = 157, 101, 8, 4
PAD = 8  # bytes of padding per row of the padded images (keeps a 4-byte format's stride 4-byte aligned)
OTHER = (en.BGR8, en.RGBA8, en.BGRA8, en.MONO8)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def pair():
    rng = np.random.Generator(np.random.PCG64(4242))
    from ug_stereomatcher_amd import synth
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 61)
    # some saturated and zero pixels, so that a channel mix-up or an alpha read cannot hide
    L.reshape(-1, 3)[rng.integers(0, W * H, 200)] = (255, 0, 17)
    return L, R


def _images(L, R, fmt):
    """The pair in `fmt` and the rgb8 pair it converts to."""
    a, b = en.encode(L, fmt), en.encode(R, fmt)
    return (a, b), (en.to_rgb8(a, fmt), en.to_rgb8(b, fmt))


class Dev:
    """Device copies of images, laid out as asked: rows padded by `pad` bytes, the first byte at `shift` past an allocation."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, img, pad=0, shift=0):
        rows = en.padded(img, pad)
        base = self.ctx.alloc(rows.nbytes + 64)
        self.bufs.append(base)
        raw = np.zeros(rows.nbytes + 64, np.uint8)
        raw[shift:shift + rows.nbytes] = rows.reshape(-1)
        self.ctx.check(self.ctx.lib.ugsm_copy_to_device(self.ctx.handle, base, raw.ctypes.data, raw.nbytes))
        return base + shift, rows.shape[1]

    def out(self, nfloats):
        p = self.ctx.alloc(4 * nfloats + 64)
        self.bufs.append(p)
        self.ctx.check(self.ctx.lib.ugsm_copy_to_device(self.ctx.handle, p, np.full(nfloats, np.nan, np.float32).ctypes.data, 4 * nfloats))
        return p

    def free(self):
        for p in self.bufs:
            self.ctx.free(p)
        self.bufs = []


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _full_device(c, fmt, imgs, pad=0, shift=0):
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        (pl, stride), (pr, _) = d.put(imgs[0], pad, shift), d.put(imgs[1], pad, shift)
        o = d.out(3 * W * H)
        c.check(c.lib.ugsm_submit_full(c.handle, 0, pl, pr, W, H, stride, o))
        c.check(c.lib.ugsm_wait(c.handle, 0))
        return c.to_host(o, (3, H, W))
    finally:
        d.free()


def _foveated_device(c, fmt, imgs, off, pad=0, shift=0):
    c.set_input_format(fmt)
    fw, fh = (int(v) for v in c.lib_fovea)
    d = Dev(c)
    try:
        (pl, stride), (pr, _) = d.put(imgs[0], pad, shift), d.put(imgs[1], pad, shift)
        o, yl, yr = d.out(3 * F * fh * fw), d.out(3 * F * fh * fw), d.out(3 * F * fh * fw)
        c.check(c.lib.ugsm_submit_foveated(c.handle, 0, pl, pr, W, H, stride, off[0], off[1], o, yl, yr))
        c.check(c.lib.ugsm_wait(c.handle, 0))
        return [c.to_host(p, (3 * F * fh * fw,)) for p in (o, yl, yr)]
    finally:
        d.free()


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(levels=LEVELS, fovea_levels=F, slots=2, batch=3)
    c.lib_fovea = lib.fovea_dims(W, H, LEVELS, F)
    yield c
    c.close()


def _layouts(fmt):
    """(pad, shift) cases: packed rows and padded rows; the four-byte formats also 1-byte misaligned (their byte-load form)."""
    cases = [(0, 0), (PAD, 0)]
    if en.BPP[fmt] == 4:
        cases.append((PAD, 1))
    return cases


@pytest.mark.parametrize("fmt", OTHER, ids=[en.NAMES[f] for f in OTHER])
def test_full_and_foveated_device_calls_equal_rgb8_on_the_conversion(lib, ctx, pair, fmt):
    """k_pyr_base (full calls) and k_pyr_base_march (foveated calls: stack and both pyramid stacks) in every layout of the format."""
    imgs, conv = _images(*pair, fmt)
    want_full = _full_device(ctx, en.RGB8, conv)
    want_fov = _foveated_device(ctx, en.RGB8, conv, (5, -3))
    for pad, shift in _layouts(fmt):
        got = _full_device(ctx, fmt, imgs, pad, shift)
        assert np.array_equal(_bits(got), _bits(want_full)), (pad, shift)
        got = _foveated_device(ctx, fmt, imgs, (5, -3), pad, shift)
        for g, w, what in zip(got, want_fov, ("stack", "pyrL", "pyrR")):
            assert np.array_equal(_bits(g), _bits(w)), (what, pad, shift)
    ctx.set_input_format(en.RGB8)


@pytest.mark.parametrize("fmt", OTHER, ids=[en.NAMES[f] for f in OTHER])
def test_two_level_pyramids_read_the_format(lib, pair, fmt):
    """levels = 2: no k_pyr_base; level 0 comes from k_rgb_planes."""
    imgs, conv = _images(*pair, fmt)
    with lib.Context(levels=2, fovea_levels=2) as c:
        want = _full_device(c, en.RGB8, conv)
        for pad, shift in _layouts(fmt):
            assert np.array_equal(_bits(_full_device(c, fmt, imgs, pad, shift)), _bits(want)), (pad, shift)


@pytest.mark.parametrize("fmt", en.FORMATS, ids=[en.NAMES[f] for f in en.FORMATS])
def test_every_format_against_the_cpu_oracle(lib, ctx, orc, pair, fmt):
    imgs, conv = _images(*pair, fmt)
    got = _full_device(ctx, fmt, imgs, PAD, 1 if en.BPP[fmt] == 4 else 0)
    ref = orc.match_full(conv[0], conv[1], LEVELS)
    rmse = float(np.sqrt(np.mean((got.astype(np.float64) - ref) ** 2)))
    assert rmse == 0.0 and np.array_equal(_bits(got), _bits(ref))
    ctx.set_input_format(en.RGB8)


@pytest.mark.parametrize("fmt", OTHER, ids=[en.NAMES[f] for f in OTHER])
def test_batch_host_managed_and_service_calls(lib, ctx, pair, fmt):
    L, R = pair
    from ug_stereomatcher_amd import synth
    L2, R2, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 62)
    (a, b), conv = _images(L, R, fmt)
    (a2, b2), conv2 = _images(L2, R2, fmt)
    want = [_full_device(ctx, en.RGB8, conv), _full_device(ctx, en.RGB8, conv2)]
    c = ctx
    # a batch of two pairs (one launch per level for both; the second pair's image 1 byte further on for a four-byte format)
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        shift = 1 if en.BPP[fmt] == 4 else 0
        (l0, stride), (r0, _) = d.put(a, PAD), d.put(b, PAD)
        (l1, _), (r1, _) = d.put(a2, PAD, shift), d.put(b2, PAD, shift)
        outs = [d.out(3 * W * H), d.out(3 * W * H)]
        c.submit_full_batch(0, [l0, l1], [r0, r1], W, H, stride, outs)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        got = [c.to_host(o, (3, H, W)) for o in outs]
    finally:
        d.free()
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w)), "batch"
    # page-locked host memory: ugsm_submit_full_host
    hl, hr = c.host_array(a.shape, np.uint8), c.host_array(b.shape, np.uint8)
    hl[...], hr[...] = a, b
    hout = c.host_array((3, H, W), np.float32)
    c.check(c.lib.ugsm_submit_full_host(c.handle, 1, hl.ctypes.data, hr.ctypes.data, W, H, hl.strides[0], hout[0].ctypes.data,
                                        hout[1].ctypes.data, hout[2].ctypes.data))
    c.check(c.lib.ugsm_wait(c.handle, 1))
    assert np.array_equal(_bits(hout), _bits(want[0])), "_host"
    # the service call from pageable memory, padded rows (ugsm_match_full)
    rowsL, rowsR = en.padded(a, PAD), en.padded(b, PAD)
    out = np.full((3, H, W), np.nan, np.float32)
    c.check(c.lib.ugsm_match_full(c.handle, rowsL.ctypes.data, rowsR.ctypes.data, W, H, rowsL.shape[1], out[0].ctypes.data, out[1].ctypes.data,
                                  out[2].ctypes.data))
    assert np.array_equal(_bits(out), _bits(want[0])), "ugsm_match_full"
    # managed queue calls (the rows compacted to bpp x W bytes), with padded input rows
    pa = en.padded(a, PAD)[:, :a[0].nbytes].reshape(a.shape)
    pb = en.padded(b, PAD)[:, :b[0].nbytes].reshape(b.shape)
    c.enqueue_full_managed(pa, pb, 1)
    c.enqueue_full_managed(a2, b2, 2)
    for k in range(2):
        done = c.next_done(True)
        assert done.tag == k + 1
        planes = np.stack(c.managed_planes(done, [(H, W)] * 3))
        assert np.array_equal(_bits(planes), _bits(want[k])), ("managed", k)
    c.set_input_format(en.RGB8)


def test_the_queue_keeps_each_pairs_format(lib, pair):
    """A burst of pairs in every format, the format changed between enqueues: each pair goes out in a call of its own format (pairs of different
    formats never share one) and comes out right; device-queue calls.  Every image lies in rows of ONE stride (4 W + PAD bytes, enough for
    every format), so that neighbouring pairs differ in their format alone: only the format in the queue's call-forming key keeps them apart."""
    L, R = pair
    with lib.Context(levels=LEVELS, fovea_levels=F, slots=2, batch=3) as c:
        want, d = {}, Dev(c)
        try:
            order = [en.RGB8, en.RGB8, en.BGR8, en.MONO8, en.MONO8, en.RGBA8, en.BGRA8, en.RGB8, en.BGR8]
            for fmt in set(order):
                want[fmt] = _full_device(c, en.RGB8, _images(L, R, fmt)[1])
            outs = []
            for k, fmt in enumerate(order):
                imgs = _images(L, R, fmt)[0]
                pad = 4 * W + PAD - imgs[0][0].nbytes
                (pl, stride), (pr, _) = d.put(imgs[0], pad), d.put(imgs[1], pad)
                assert stride == 4 * W + PAD
                o = d.out(3 * W * H)
                outs.append(o)
                c.set_input_format(fmt)
                c.enqueue_full(pl, pr, W, H, stride, o, k)
            c.set_input_format(en.RGB8)
            done = c.drain()
            assert [x.tag for x in done] == list(range(len(order)))
            assert max(x.call_pairs for x in done) > 1  # (the queue did batch pairs of one format)
            calls = {}
            for x in done:
                calls.setdefault(int(x.call_index), set()).add(order[x.tag])
            assert all(len(v) == 1 for v in calls.values()), calls
            for k, fmt in enumerate(order):
                assert np.array_equal(_bits(c.to_host(outs[k], (3, H, W))), _bits(want[fmt])), (k, en.NAMES[fmt])
        finally:
            d.free()


def test_setter_errors_and_stride_checks(lib, ctx, pair):
    c = ctx
    c.set_input_format(en.BGRA8)
    for bad in (-1, 5, 99):
        with pytest.raises(lib.UgsmError) as e:
            c.set_input_format(bad)
        assert e.value.status == lib.UGSM_ERR_BAD_ARG
        assert c.input_format == en.BGRA8
    import ctypes as C
    out = C.c_int(-7)
    assert c.lib.ugsm_get_input_format(None, C.byref(out)) == lib.UGSM_ERR_BAD_ARG
    assert c.lib.ugsm_set_input_format(None, 0) == lib.UGSM_ERR_BAD_ARG
    d = Dev(c)
    try:
        for fmt in en.FORMATS:
            c.set_input_format(fmt)
            img = en.encode(pair[0], fmt)
            p, stride = d.put(img)
            o = d.out(3 * W * H)
            assert stride == en.BPP[fmt] * W
            assert c.lib.ugsm_submit_full(c.handle, 0, p, p, W, H, stride - 1, o) == lib.UGSM_ERR_SIZE_MISMATCH
            assert c.lib.ugsm_enqueue_full(c.handle, p, p, W, H, stride - 1, o, 0) == lib.UGSM_ERR_SIZE_MISMATCH
            assert c.lib.ugsm_stage_pyramid(c.handle, p, W, H, stride - 1, 0, o) == lib.UGSM_ERR_SIZE_MISMATCH
            host = np.zeros((H, stride), np.uint8)
            res = np.zeros((3, H, W), np.float32)
            assert c.lib.ugsm_match_full(c.handle, host.ctypes.data, host.ctypes.data, W, H, stride - 1, res[0].ctypes.data, res[1].ctypes.data,
                                         res[2].ctypes.data) == lib.UGSM_ERR_SIZE_MISMATCH
            # the NumPy-taking methods check the shape against the format
            wrong = np.zeros((H, W, 3) if en.BPP[fmt] != 3 else (H, W), np.uint8)
            with pytest.raises(lib.UgsmError):
                c.enqueue_full_managed(wrong, wrong, 0)
    finally:
        d.free()
        c.set_input_format(en.RGB8)


def _stage_pyramid(c, fmt, img, level):
    c.set_input_format(fmt)
    d = Dev(c)
    try:
        p, stride = d.put(img, PAD)
        w, h = (int(v[level]) for v in c_level_dims(W, H))
        o = d.out(3 * w * h)
        c.check(c.lib.ugsm_stage_pyramid(c.handle, p, W, H, stride, level, o))
        return c.to_host(o, (3, h, w))
    finally:
        d.free()


def c_level_dims(W_, H_):
    from ug_stereomatcher_amd import _lib
    return _lib.level_dims(W_, H_, LEVELS)


def test_stage_pyramid_mono8_levels_are_three_equal_planes(lib, ctx, pair):
    """ugsm_stage_pyramid captures the format too; mono8's one computed channel lands in all three planes (levels 0, 1, 2 of k_pyr_base and a
    level made from them)."""
    mono = en.encode(pair[0], en.MONO8)
    for level in (0, 1, 2, 3):
        got = _stage_pyramid(ctx, en.MONO8, mono, level)
        want = _stage_pyramid(ctx, en.RGB8, en.to_rgb8(mono, en.MONO8), level)
        assert np.array_equal(_bits(got), _bits(want)), level
        assert np.array_equal(_bits(got[0]), _bits(got[1])) and np.array_equal(_bits(got[0]), _bits(got[2]))
    ctx.set_input_format(en.RGB8)


def _cloud_calls(c, lib, fmt, img, planes, stack, compact):
    """The four cloud calls coloured from `img` in `fmt`: (count, record bytes) of each."""
    c.set_input_format(fmt)
    d = Dev(c)
    res = []
    try:
        p_img, stride = d.put(img, PAD, 1 if en.BPP[fmt] == 4 else 0)
        dx, dy, cf = (c.to_device(a) for a in planes)
        sx, sy, sc = (c.to_device(a) for a in stack)
        d.bufs += [dx, dy, cf, sx, sy, sc]
        fw, fh = (int(v) for v in c.lib_fovea)
        left, upper, scale = lib.fovea_mapping(W, H, 1)
        params = lib.cloud_params(format=cn.PCL32, compact=compact, min_conf=0.2 if compact else None)
        cap = W * H
        for kind in ("dense", "fovea", "resized", "resized_fovea"):
            pts = d.out(8 * (cap + 16))
            cnt = c.to_device(np.full(1, -7, np.int64))
            d.bufs.append(cnt)
            if kind == "dense":
                n = c.point_cloud(dx, dy, cf, p_img, W, H, stride, P1, P2A, params, pts, cap, cnt)
            elif kind == "fovea":
                n = c.point_cloud_fovea(sx, sy, sc, fw, fh, 1, left, upper, scale, p_img, W, H, stride, P1, P2A, params, pts, cap, cnt)
            elif kind == "resized":
                n = c.point_cloud_resized(dx, dy, cf, p_img, W, H, stride, P1, P2A, 0.5, params, pts, cap, cnt)
            else:
                n = c.point_cloud_resized_fovea(sx, sy, sc, fw, fh, 1, left, upper, scale, p_img, W, H, stride, P1, P2A, 0.5, params, pts, cap, cnt,
                                                colour_mapped=True)
            res.append((n, c.to_host(pts, (min(n, cap) * 32,), np.uint8)))
    finally:
        d.free()
        c.set_input_format(en.RGB8)
    return res


@pytest.mark.parametrize("fmt", (en.BGR8, en.RGBA8, en.MONO8), ids=("bgr8", "rgba8", "mono8"))
def test_the_four_cloud_calls_colour_from_the_format(lib, ctx, pair, fmt):
    rng = np.random.Generator(np.random.PCG64(99 + fmt))
    planes = (rng.normal(-40, 25, (H, W)).astype(np.float32), rng.normal(0, 2, (H, W)).astype(np.float32),
              rng.uniform(0, 1, (H, W)).astype(np.float32))
    fw, fh = (int(v) for v in ctx.lib_fovea)
    stack = (rng.normal(-20, 9, (F * fh, fw)).astype(np.float32), rng.normal(0, 1, (F * fh, fw)).astype(np.float32),
             rng.uniform(0, 1, (F * fh, fw)).astype(np.float32))
    img = en.encode(pair[0], fmt)
    conv = en.to_rgb8(img, fmt)
    for compact in (False, True):
        got = _cloud_calls(ctx, lib, fmt, img, planes, stack, compact)
        want = _cloud_calls(ctx, lib, en.RGB8, conv, planes, stack, compact)
        for k, ((n, g), (m, w)) in enumerate(zip(got, want)):
            assert n == m and np.array_equal(g, w), (k, compact)
    # the colour word itself: the dense cloud's is R << 16 | G << 8 | B of the converted pixel (mono8: v * 0x010101), column-major
    n, raw = _cloud_calls(ctx, lib, fmt, img, planes, stack, False)[0]
    words = raw.view(cn.DTYPES[cn.PCL32])["rgb"]
    assert np.array_equal(words, cn.column_major(cn.colour_word(conv), 1))
    if fmt == en.MONO8:
        assert np.array_equal(words, cn.column_major(img.astype(np.uint32) * 0x010101, 1))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_fovea_shard_step_reads_bgr8(lib):
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               UGSM_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("UGSM_DIST_BACKEND", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shard_input_format_child.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert "SHARD_FORMAT_OK" in r.stdout, tail
