"""The merged cloud of several fovea windows of one pair on the device (ugsm_point_cloud_fovea_multi) against the CPU restatement
(tests/multi_cloud_np.py), against the per-level call it is defined by and against ugsm_point_cloud_fovea_all for one window: byte for
byte, a NaN X, Y or Z equal to any NaN."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import encode_np as en
import multi_cloud_np as mn
import stack_cloud_np as sn
from test_gpu_cloud import P1, P2, P2A, _inputs, _poisoned, _read
from test_multi_cloud_host import CASES, LEVELS, bad_argument_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def _random_stacks(rng, W, H, F, n):
    """n stacks (3, F, fovH, fovW) salted with NaN / inf (level F-1 differs between them too: the cloud reads stack 0's), and the image."""
    fw, fh = sn.fovea_dims(W, H, F)
    stacks = [np.stack([a.reshape(F, fh, fw) for a in _inputs(rng, fw, F * fh)[:3]]) for _ in range(n)]
    return stacks, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _planes(d_stack, W, H, F):
    fw, fh = sn.fovea_dims(W, H, F)
    plane = F * fw * fh * 4
    return d_stack, d_stack + plane, d_stack + 2 * plane


def _multi(c, lib, d_stacks, d_rgb, W, H, offsets, stride, P2_, fmt, s, compact, cap=None, extra=64, slot=0, counts=True, **kw):
    """One merged cloud into a poisoned buffer -> (count, the records written, the per-entry counts); checks the bytes behind them."""
    F, E = c.cfg.fovea_levels, (c.cfg.fovea_levels - 1) * len(d_stacks) + 1
    params = lib.cloud_params(sampling=s, format=fmt, compact=compact, **kw)
    if cap is None:
        cap = lib.fovea_multi_cloud_points(W, H, c.cfg.levels, F, offsets, s)
    d_pts = _poisoned(c, (cap + extra) * cn.DTYPES[fmt].itemsize)
    d_cnt = c.to_device(np.full(1, -7, np.int64))
    d_ent = c.to_device(np.full(E + 1, -7, np.int64)) if counts else None
    try:
        got = c.point_cloud_fovea_multi(d_stacks, W, H, offsets, d_rgb, stride, P1, P2_, params, d_pts, cap, d_cnt, d_ent, slot=slot)
        n, per = got if counts else (got, None)
        if counts:
            assert c.to_host(d_ent, (E + 1,), np.int64)[E] == -7, "a word past the entry counts was touched"
        return n, _read(c, lib, d_pts, cap, extra, fmt, n), per
    finally:
        for p in (d_pts, d_cnt, d_ent):
            if p is not None:
                c.free(p)


def _per_entry(c, lib, d_stacks, d_rgb, W, H, offsets, fmt, s, stride=None, P2_=P2A):
    """The dense cloud of every entry from ugsm_point_cloud_fovea with ugsm_fovea_level_mapping's numbers: a list of record arrays."""
    levels, F = c.cfg.levels, c.cfg.fovea_levels
    fw, fh = sn.fovea_dims(W, H, F)
    d_pts, d_cnt = c.alloc(fw * fh * 32), c.alloc(8)
    out = []
    try:
        for j, k in mn.entries(F, len(d_stacks)):
            left, upper, scale = lib.fovea_level_mapping(W, H, levels, F, k, offsets[j])
            n = c.point_cloud_fovea(*_planes(d_stacks[j], W, H, F), fw, fh, k, left, upper, scale, d_rgb, W, H, stride or 3 * W, P1, P2_,
                                    lib.cloud_params(sampling=s, format=fmt), d_pts, fw * fh, d_cnt)
            assert n == cn.cloud_points(fw, fh, s)
            out.append(c.cloud_to_host(d_pts, n, fmt))
    finally:
        c.free(d_pts)
        c.free(d_cnt)
    return out


def _z_window(orc, stacks, W, H, F, offsets):
    zs = np.concatenate([orc.triangulate_fovea(stacks[j][0], stacks[j][1], k, *sn.level_mapping(W, H, F, k, offsets[j]), P1, P2A)[2].reshape(-1)
                         for j, k in mn.entries(F, len(stacks))])
    return tuple(float(np.percentile(zs[np.isfinite(zs)], q)) for q in (10, 90))


@pytest.mark.parametrize("W,H,F,offsets", [c[:4] for c in CASES])
def test_random_stacks_match_the_restatement(lib, orc, W, H, F, offsets):
    """Both record formats x dense / compact x sampling 1 and 3 on stacks with NaN, inf and wild disparities: the count, the bytes, the
    per-entry counts and the poison behind the records.  The shapes: fovW 18 (one strip), 166 (six strips, the last ragged), fovH 84 and
    125 (two chunks), tiles wholly inside a rectangle, empty entries.  The pixels whose integer conversion C leaves undefined
    (stack_cloud_np's note) take X, Y, Z from ugsm_point_cloud_fovea's record for the pixel."""
    n = len(offsets)
    rng = np.random.Generator(np.random.PCG64(W * 100 + F * 10 + n))
    stacks, rgb = _random_stacks(rng, W, H, F, n)
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        zlo, zhi = _z_window(orc, stacks, W, H, F, offsets)
        undef = sum(int(sn.undefined_conversion(t[0], t[1], k).sum()) for t in stacks for k in range(F))
        assert 0 < undef < sum(t[0].size for t in stacks) // 10
        for s in (1, 3):
            for fmt in (cn.PCL32, cn.XYZRGB16):
                und = _per_entry(c, lib, d_stacks, d_rgb, W, H, offsets, fmt, s)
                for compact in (False, True):
                    kw = dict(min_conf=0.3, z_min=zlo, z_max=zhi) if compact else {}
                    exp, exp_per = mn.cloud_fovea_multi(orc, stacks, rgb, offsets, P1, P2A, s=s, fmt=fmt, compact=compact, undefined=und, **kw)
                    cnt, got, per = _multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, fmt, s, compact, **kw)
                    what = f"{W}x{H} F={F} n={n} s={s} fmt={fmt} compact={compact}"
                    assert cnt == exp.size and per == exp_per, what
                    if not compact:
                        assert (cnt, per) == lib.fovea_multi_cloud_points(W, H, LEVELS[F], F, offsets, s, per_entry=True)
                    cn.assert_cloud_equal(got, exp, what)
        # a compact cloud whose confidence test is off (min_conf -inf: the confidence planes are not read), without the entry counts
        exp, _ = mn.cloud_fovea_multi(orc, stacks, rgb, offsets, P1, P2A, fmt=cn.XYZRGB16, compact=True, use_conf=False,
                                      undefined=_per_entry(c, lib, d_stacks, d_rgb, W, H, offsets, cn.XYZRGB16, 1))
        cnt, got, _ = _multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, cn.XYZRGB16, 1, True, counts=False)
        assert cnt == exp.size
        cn.assert_cloud_equal(got, exp, "compact, no confidence test, no entry counts")
        for p in d_stacks + [d_rgb]:
            c.free(p)


def test_sixteen_windows(lib, orc):
    """160 x 120, F = 4, sixteen offsets on a grid: E = 49 entries, more than the 32 the level-count reduction of the one-stack cloud
    handles."""
    W, H, F = 160, 120, 4
    offsets = [(-45 + 30 * x, -33 + 22 * y) for y in range(4) for x in range(4)]
    rng = np.random.Generator(np.random.PCG64(16))
    stacks, rgb = _random_stacks(rng, W, H, F, 16)
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        for fmt, compact, kw in ((cn.PCL32, False, {}), (cn.XYZRGB16, True, dict(min_conf=0.3))):
            und = _per_entry(c, lib, d_stacks, d_rgb, W, H, offsets, fmt, 1)
            exp, exp_per = mn.cloud_fovea_multi(orc, stacks, rgb, offsets, P1, P2A, fmt=fmt, compact=compact, undefined=und, **kw)
            cnt, got, per = _multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, fmt, 1, compact, **kw)
            assert len(per) == 49 and cnt == exp.size and per == exp_per
            cn.assert_cloud_equal(got, exp, f"sixteen windows, compact={compact}")
        for p in d_stacks + [d_rgb]:
            c.free(p)


def test_one_window_is_the_stack_cloud_byte_for_byte(lib):
    W, H, F, off = 320, 240, 4, (-60, 40)
    rng = np.random.Generator(np.random.PCG64(21))
    stacks, rgb = _random_stacks(rng, W, H, F, 1)
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stack, d_rgb = c.to_device(stacks[0]), c.to_device(rgb)
        cap = lib.fovea_cloud_points(W, H, LEVELS[F], F, off)
        d_pts, d_cnt, d_lvl = c.alloc(cap * 32), c.alloc(8), c.alloc(8 * F)
        for fmt in (cn.PCL32, cn.XYZRGB16):
            for s in (1, 3):
                for compact, kw in ((False, {}), (True, dict(min_conf=0.4, z_min=-1e3, z_max=1e3))):
                    n0, per0 = c.point_cloud_fovea_all(*_planes(d_stack, W, H, F), W, H, off, d_rgb, 3 * W, P1, P2A,
                                                       lib.cloud_params(sampling=s, format=fmt, compact=compact, **kw), d_pts, cap, d_cnt, d_lvl)
                    ref = c.cloud_to_host(d_pts, n0, fmt)
                    n1, got, per1 = _multi(c, lib, [d_stack], d_rgb, W, H, [off], 3 * W, P2A, fmt, s, compact, **kw)
                    assert (n1, per1) == (n0, per0) and got.tobytes() == ref.tobytes(), (fmt, s, compact)
        for p in (d_stack, d_rgb, d_pts, d_cnt, d_lvl):
            c.free(p)


def test_merged_cloud_is_the_per_level_clouds_without_the_left_out_records(lib):
    """ugsm_point_cloud_fovea per entry with ugsm_fovea_level_mapping's numbers, the left-out records dropped on the host: concatenated,
    that is the merged cloud byte for byte, dense, in both formats."""
    W, H, F, offsets = CASES[2][:4]
    rng = np.random.Generator(np.random.PCG64(11))
    stacks, rgb = _random_stacks(rng, W, H, F, len(offsets))
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        for s in (1, 2):
            for fmt in (cn.PCL32, cn.XYZRGB16):
                item = cn.DTYPES[fmt].itemsize
                dense = _per_entry(c, lib, d_stacks, d_rgb, W, H, offsets, fmt, s)
                parts = [d.view(np.uint8).reshape(-1, item)[~cn.column_major(mn.left_out(W, H, F, offsets, j, k), s)]
                         for d, (j, k) in zip(dense, mn.entries(F, len(offsets)))]
                exp = np.concatenate(parts).reshape(-1)
                n, got, per = _multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, fmt, s, False)
                assert n * item == exp.size and per == [p.shape[0] for p in parts]
                assert np.array_equal(got.view(np.uint8), exp), f"s={s} fmt={fmt}"
        for p in d_stacks + [d_rgb]:
            c.free(p)


def test_cap_below_count_writes_exactly_cap_records(lib, orc):
    W, H, F, offsets = CASES[2][:4]
    rng = np.random.Generator(np.random.PCG64(5))
    stacks, rgb = _random_stacks(rng, W, H, F, len(offsets))
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        for fmt in (cn.PCL32, cn.XYZRGB16):
            und = _per_entry(c, lib, d_stacks, d_rgb, W, H, offsets, fmt, 1)
            for compact, kw in ((False, {}), (True, dict(min_conf=0.5))):
                exp, exp_per = mn.cloud_fovea_multi(orc, stacks, rgb, offsets, P1, P2A, fmt=fmt, compact=compact, undefined=und, **kw)
                for cap in (0, 1, 97, exp_per[0] + 5, exp.size // 2 + 3, exp.size - 1):
                    n, got, per = _multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, fmt, 1, compact, cap=cap, extra=100, **kw)
                    assert n == exp.size and got.size == cap and per == exp_per   # (the counts are the cloud's, not what was written)
                    cn.assert_cloud_equal(got, exp[:cap], f"cap {cap} fmt={fmt} compact={compact}")
        for p in d_stacks + [d_rgb]:
            c.free(p)


def test_compact_cloud_is_deterministic(lib):
    W, H, F, offsets = CASES[4][:4]
    rng = np.random.Generator(np.random.PCG64(6))
    stacks, rgb = _random_stacks(rng, W, H, F, len(offsets))
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        runs = [_multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, cn.PCL32, 1, True, min_conf=0.4) for _ in range(2)]
        assert runs[0][0] > 0
        assert runs[1][0] == runs[0][0] and runs[1][2] == runs[0][2] and runs[1][1].tobytes() == runs[0][1].tobytes()
        for p in d_stacks + [d_rgb]:
            c.free(p)


def test_bgra8_image_gives_the_cloud_of_its_rgb8_conversion(lib):
    W, H, F, offsets = CASES[2][:4]
    rng = np.random.Generator(np.random.PCG64(8))
    stacks, rgb = _random_stacks(rng, W, H, F, len(offsets))
    img = en.encode(rgb, en.BGRA8)
    assert np.array_equal(en.to_rgb8(img, en.BGRA8), rgb)
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        d_stacks, d_rgb, d_img = [c.to_device(t) for t in stacks], c.to_device(rgb), c.to_device(img)
        n0, rec0, per0 = _multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, cn.PCL32, 1, False)
        c.set_input_format(en.BGRA8)
        n1, rec1, per1 = _multi(c, lib, d_stacks, d_img, W, H, offsets, 4 * W, P2A, cn.PCL32, 1, False)
        n2, rec2, per2 = _multi(c, lib, d_stacks, d_img, W, H, offsets, 4 * W, P2A, cn.XYZRGB16, 1, True, min_conf=0.3)
        c.set_input_format(en.RGB8)
        n3, rec3, per3 = _multi(c, lib, d_stacks, d_rgb, W, H, offsets, 3 * W, P2A, cn.XYZRGB16, 1, True, min_conf=0.3)
        assert (n0, per0) == (n1, per1) and rec0.tobytes() == rec1.tobytes()
        assert (n2, per2) == (n3, per3) and rec2.tobytes() == rec3.tobytes()
        for p in d_stacks + [d_rgb, d_img]:
            c.free(p)


def test_end_to_end_after_submit_foveated_multi_on_the_same_slot(lib, orc):
    """ugsm_submit_foveated_multi at 640 x 480, 10 / 4 levels, three windows, then the merged cloud on the same slot with no wait in
    between (stream order), against the restatement on the oracle's stacks."""
    from ug_stereomatcher_amd import synth
    W, H, levels, F, offsets = 640, 480, 10, 4, [(-70, 30), (0, 0), (55, -25)]
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 33)
    stacks = [orc.match_foveated(L, R, levels, F, ox, oy)[0] for ox, oy in offsets]
    exp, exp_per = mn.cloud_fovea_multi(orc, stacks, L, offsets, P1, P2, compact=True, min_conf=0.2)
    dense, dense_per = mn.cloud_fovea_multi(orc, stacks, L, offsets, P1, P2)
    E = (F - 1) * len(offsets) + 1
    with lib.Context(levels=levels, fovea_levels=F, slots=2) as c:
        pL, pR = c.to_device(L), c.to_device(R)
        d_stacks = [c.alloc(stacks[0].nbytes) for _ in offsets]
        d_pts, d_cnt, d_ent = c.alloc(dense.size * 32), c.alloc(8), c.alloc(8 * E)
        for params, want, want_per in ((lib.cloud_params(compact=True, min_conf=0.2), exp, exp_per), (lib.cloud_params(), dense, dense_per)):
            c.submit_foveated_multi(1, pL, pR, W, H, L.strides[0], offsets, d_stacks)
            n, per = c.point_cloud_fovea_multi(d_stacks, W, H, offsets, pL, L.strides[0], P1, P2, params, d_pts, dense.size, d_cnt, d_ent, slot=1)
            assert n == want.size and per == want_per
            cn.assert_cloud_equal(c.cloud_to_host(d_pts, n), want, f"640 x 480 after submit_foveated_multi, compact={params.compact}")
        for p in [pL, pR, d_pts, d_cnt, d_ent] + d_stacks:
            c.free(p)


def test_bad_arguments_on_a_live_context(lib):
    """Every refusal of the host test on a live context with real buffers (large enough that nothing could be touched out of bounds
    even if a check were missing), a null entry, a context whose stack has one level, a slot that does not exist; then calls that pass."""
    W, H, F = 320, 240, 4
    fw, fh = sn.fovea_dims(W, H, F)
    P = (C.c_double * 12)(*P1.reshape(12))
    with lib.Context(levels=LEVELS[F], fovea_levels=F) as c:
        stack = 3 * F * fw * fh * 4
        bufs = dict(dx=c.to_device(np.zeros(stack, np.uint8)), dy=c.to_device(np.zeros(stack, np.uint8)), rgb=c.to_device(np.zeros(3 * W * H, np.uint8)),
                    points=c.alloc(2 * F * fw * fh * 32), count=c.alloc(8), entry_counts=c.alloc(8 * (2 * (F - 1) + 1)))
        so = lib.load()

        def call(handle=c.handle, slot=0, **over):
            a = dict(bufs, W=W, H=H, stride=3 * W, P1=P, P2=P, p=lib.cloud_params(), cap=100, n=2, stacks=True)
            if over.get("points") is not None:
                over["points"] = bufs["points"] + 8            # (the misaligned cases, at real addresses)
            if "level_counts" in over:
                over["entry_counts"] = over.pop("level_counts")
            if over.get("entry_counts") is not None:
                over["entry_counts"] = bufs["entry_counts"] + 4
            if over.get("stride") == 191:
                over["stride"] = 3 * W - 1                     # (one byte short of this image's rows)
            a.update(over)
            p = C.byref(a["p"]) if a["p"] is not None else None
            stacks = (C.c_void_p * 17)(a["dx"], a["dy"], *([bufs["dx"]] * 15)) if a["stacks"] else None
            return so.ugsm_point_cloud_fovea_multi(handle, slot, a["n"], stacks, a["W"], a["H"], None, None, a["rgb"], a["stride"], a["P1"], a["P2"],
                                                   p, a["points"], a["cap"], a["count"], a["entry_counts"])
        try:
            for name, over in bad_argument_cases(lib):
                assert call(**dict(over)) == lib.UGSM_ERR_BAD_ARG, name
            assert call(slot=5) == lib.UGSM_ERR_BAD_ARG                       # (no such slot)
            assert call(W=2, H=2, stride=6) != lib.UGSM_OK                    # (too small for the stack's four levels)
            with lib.Context(levels=8, fovea_levels=1) as one:                # a one-level stack is the full frame: ugsm_point_cloud
                assert call(handle=one.handle) == lib.UGSM_ERR_BAD_ARG
            c.check(so.ugsm_wait(c.handle, 0))
            assert call() == lib.UGSM_OK and call(entry_counts=None) == lib.UGSM_OK and call(n=1) == lib.UGSM_OK
            c.check(so.ugsm_wait(c.handle, 0))
            assert c.to_host(bufs["count"], (1,), np.int64)[0] == lib.fovea_cloud_points(W, H, LEVELS[F], F)
        finally:
            for p in bufs.values():
                c.free(p)


def test_nine_calls_back_to_back_take_turns_on_the_upload_ring(lib):
    """320 x 240, two windows: nine ugsm_point_cloud_fovea_multi calls on one slot with no wait between them, each into its own poisoned
    point buffer and count words, rotating through three offset sets (and dense / compact), so that call k and call k - 4 -- which fill the
    same page-locked copy of the table -- never share a table: a stale copy shows as a wrong cloud.  After one ugsm_wait every call's
    records (and the poison behind them), count and entry counts equal byte for byte what the same call gave when made alone and waited
    for on that context."""
    W, H, F = CASES[2][:3]
    sets = [[(-60, 40), (0, 0)], [(25, 10), (-30, -20)], [(40, -35), (10, 50)]]
    n, E, fmt, extra = 2, (F - 1) * 2 + 1, cn.PCL32, 64
    item = cn.DTYPES[fmt].itemsize
    rng = np.random.Generator(np.random.PCG64(44))
    stacks, rgb = _random_stacks(rng, W, H, F, n)
    dp = C.POINTER(C.c_double)
    p1, p2 = (np.ascontiguousarray(P, np.float64).reshape(12) for P in (P1, P2A))
    with lib.Context(levels=LEVELS[F], fovea_levels=F, slots=1) as c:
        so, h = c.lib, c.handle
        d_stacks, d_rgb = [c.to_device(t) for t in stacks], c.to_device(rgb)
        calls = [(sets[k % 3], bool(k % 2)) for k in range(9)]
        assert all(calls[k][0] != calls[k - 4][0] for k in range(4, 9))
        caps = [lib.fovea_multi_cloud_points(W, H, LEVELS[F], F, offs, 1) for offs, _ in calls]
        params = [lib.cloud_params(format=fmt, compact=True, min_conf=0.3) if compact else lib.cloud_params(format=fmt) for _, compact in calls]
        held = []

        def enqueue(k):
            bufs = (_poisoned(c, (caps[k] + extra) * item), c.to_device(np.full(1, -7, np.int64)), c.to_device(np.full(E + 1, -7, np.int64)))
            held.extend(bufs)
            ox, oy = c._offsets(calls[k][0], n)
            c.check(so.ugsm_point_cloud_fovea_multi(h, 0, n, c._ptrs(d_stacks), W, H, ox, oy, d_rgb, 3 * W, p1.ctypes.data_as(dp), p2.ctypes.data_as(dp),
                                                    C.byref(params[k]), bufs[0], caps[k], bufs[1], bufs[2]))
            return bufs

        def result(k, bufs):
            return (c.to_host(bufs[0], ((caps[k] + extra) * item,), np.uint8).tobytes(), c.to_host(bufs[1], (1,), np.int64).tobytes(),
                    c.to_host(bufs[2], (E + 1,), np.int64).tobytes())
        try:
            alone = []
            for k in range(9):
                bufs = enqueue(k)
                c.check(so.ugsm_wait(h, 0))
                alone.append(result(k, bufs))
            # the premise: per form, the three offset sets give three different clouds (and every call wrote one)
            for form in ((0, 2, 4), (1, 3, 5)):
                assert len({alone[k][0] for k in form}) == 3 and len({alone[k][2] for k in form}) == 3
            assert all(0 < np.frombuffer(a[1], np.int64)[0] <= cap for a, cap in zip(alone, caps))
            queued = [enqueue(k) for k in range(9)]
            c.check(so.ugsm_wait(h, 0))
            for k in range(9):
                got = result(k, queued[k])
                assert got[1] == alone[k][1] and got[2] == alone[k][2], f"call {k}: the count or the entry counts"
                assert got[0] == alone[k][0], f"call {k}: the records"
        finally:
            for p in held + d_stacks + [d_rgb]:
                c.free(p)
