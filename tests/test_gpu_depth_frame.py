"""The depth image of the whole frame straight from a fovea stack (ugsm_depth_image_fovea_full, ugsm_depth_image_fovea_multi,
ugsm_match_foveated_depth; include/ugsm.h) against (a) the composition it replaces on the device -- ugsm_reconstruct_full[_multi] into a
field, then ugsm_depth_image on the field's planes -- and (b) the CPU statement depth_np.depth_of_z(orc.triangulate(reconstruction)[2]), the
reconstruction being the oracle's hierarchicalDisparity (one window) or tests/reconstruct_multi_np.py (several).  Everything bit for bit,
the NaN's payload and the count of valid pixels included.

Stacks are synthetic: level l holds N(-40, 12) / s^l in dx, N(0, 2) / s^l in dy and U(0, 1) / s^l in the confidence, so that the
reconstructed field has the full-resolution cases' distribution wherever it comes from.  Every call runs on caller-owned memory between guard
bands (tests/guarded.py for the stacks, test_gpu_depth._Band for the image).  Every filtered and every 16U case of the single-window test
asserts on the restatement that both branches are taken (depth_np.assert_both_branches)."""
import ctypes as C

import numpy as np
import pytest

import depth_np as dn
import lens_np as ln
import reconstruct_multi_np as rm
from guarded import POISON, Guards
from test_gpu_cloud import P1, P2
from test_gpu_depth import BAND, WILD, _Band, params_of, window

pytestmark = pytest.mark.gpu

S = np.float32(1.41421356)
FW, FH, FLV, FF = 160, 120, 8, 4      # the fovea cases' frame, levels and fovea levels
OW, OH, OLV, OF = 67, 41, 5, 3        # odd width, W * H no multiple of 8
CORNER = (1000, 1000)                 # clamps the window against the frame's bottom right corner at every level


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def fctx(lib):
    c = lib.Context(levels=FLV, fovea_levels=FF)
    yield c
    c.close()


@pytest.fixture(scope="module")
def octx(lib):
    c = lib.Context(levels=OLV, fovea_levels=OF)
    yield c
    c.close()


def make_stack(lib, W, H, levels, F, seed, nan_conf=60):
    """One (3, F, fovH, fovW) stack; nan_conf: one confidence in that many is a NaN (0: none)."""
    fw, fh = lib.fovea_dims(W, H, levels, F)
    rng = np.random.Generator(np.random.PCG64(W * 7919 + H * 31 + 1000 * F + seed))
    st = np.empty((3, F, fh, fw), np.float32)
    for l in range(F):
        k = S ** np.float32(l)
        st[0, l] = rng.normal(-40, 12, (fh, fw)).astype(np.float32) / k
        st[1, l] = rng.normal(0, 2, (fh, fw)).astype(np.float32) / k
        st[2, l] = rng.uniform(0, 1, (fh, fw)).astype(np.float32) / k
    if nan_conf:
        st[2].flat[rng.integers(0, st[2].size, st[2].size // nan_conf)] = np.nan
    return st


def field_of(orc, stacks, W, H, levels, offsets):
    """The CPU reconstruction: the oracle's for one window, the NumPy statement for several."""
    if len(stacks) == 1:
        return orc.reconstruct_full(stacks[0], W, H, levels, int(offsets[0][0]), int(offsets[0][1]))
    return rm.reconstruct_multi(orc, stacks, W, H, levels, offsets)


def restated(orc, field, P1_, P2_, conf=True, factor=1.0, **kw):
    z = orc.triangulate(field[0], field[1], P1_, P2_)[2]
    return dn.depth_of_z(z, conf=field[2] if conf else None, factor=factor, **kw)


def fused(ctx, lib, stacks, offsets, W, H, P1_, P2_, params, conf=True, multi=None, in_shift=0, out_shift=0, what=""):
    """The fused call on guarded buffers -> (image, count).  One stack and multi not True: ugsm_depth_image_fovea_full on three planes of
    their own (conf False: d_stackc NULL); else ugsm_depth_image_fovea_multi on one buffer per stack."""
    multi = len(stacks) > 1 if multi is None else multi
    dw, dh = lib.depth_image_size(W, H, params.factor)
    dtype = lib.DEPTH_DTYPES[params.format]
    g, band = Guards(ctx), _Band(ctx, dw * dh * dtype.itemsize, out_shift)
    d_valid = ctx.to_device(np.full(1, 0xDEADBEEF, np.uint64))
    try:
        if multi:
            n = ctx.depth_image_fovea_multi([g.inp(st, in_shift) for st in stacks], W, H, offsets, P1_, P2_, params, band.ptr, d_valid)
        else:
            st = stacks[0]
            n = ctx.depth_image_fovea_full(g.inp(st[0], in_shift), g.inp(st[1], in_shift), g.inp(st[2], in_shift) if conf else None, W, H,
                                           offsets[0], P1_, P2_, params, band.ptr, d_valid)
        return band.read(dtype, (dh, dw), what), n
    finally:
        g.done(what)
        band.free()
        ctx.free(d_valid)


def composed(ctx, lib, stacks, offsets, W, H, P1_, P2_, params, conf=True):
    """(a): ugsm_reconstruct_full[_multi] into a field, then ugsm_depth_image on its planes -> (image, count)."""
    dw, dh = lib.depth_image_size(W, H, params.factor)
    dtype = lib.DEPTH_DTYPES[params.format]
    n = W * H
    d_st = [ctx.to_device(st) for st in stacks]
    d_field, d_img, d_valid = ctx.alloc(3 * n * 4), ctx.alloc(dw * dh * dtype.itemsize), ctx.alloc(8)
    try:
        if len(stacks) == 1:
            plane = stacks[0][0].size * 4
            ctx.reconstruct_full(d_st[0], d_st[0] + plane, d_st[0] + 2 * plane, W, H, d_field, int(offsets[0][0]), int(offsets[0][1]))
        else:
            ctx.reconstruct_full_multi(d_st, W, H, d_field, offsets)
        cnt = ctx.depth_image(d_field, d_field + 4 * n, d_field + 8 * n if conf else None, W, H, P1_, P2_, params, d_img, d_valid)
        return ctx.to_host(d_img, (dh, dw), dtype), cnt
    finally:
        for p in d_st + [d_field, d_img, d_valid]:
            ctx.free(p)


def check_three_ways(ctx, lib, orc, stacks, offsets, W, H, levels, params, kw, what, conf=True, both=False, shifts=((0, 0),), P=(P1, P2), field=None,
                     multi=None):
    """fused == composition == restatement, image and count, at every (stack shift, image shift)."""
    field = field_of(orc, stacks, W, H, levels, offsets) if field is None else field
    exp, valid = restated(orc, field, P[0], P[1], conf=conf, factor=params.factor, **kw)
    if both:
        dn.assert_both_branches(valid, what)
    want, nw = composed(ctx, lib, stacks, offsets, W, H, P[0], P[1], params, conf=conf)
    dn.assert_image_equal(want, exp, f"{what}: the composition vs the restatement")
    assert nw == int(valid.sum()), what
    for in_shift, out_shift in shifts:
        got, n = fused(ctx, lib, stacks, offsets, W, H, P[0], P[1], params, conf=conf, multi=multi, in_shift=in_shift, out_shift=out_shift,
                       what=f"{what} shifts {in_shift}/{out_shift}")
        dn.assert_image_equal(got, want, f"{what}, shifts {in_shift}/{out_shift}: fused vs the composition")
        assert n == nw, f"{what}: count {n} vs {nw}"
    return field


def filtered(orc, field, P=(P1, P2)):
    """(label, keyword arguments, with the confidence, filtered) of a reconstruction: the window and the unit from the restatement's own Z."""
    z = orc.triangulate(field[0], field[1], P[0], P[1])[2]
    zlo, zhi = window(z)
    unit = 60.0 / float(np.percentile(z[np.isfinite(z) & (z > 0)], 80))      # the farthest fifth lies past 65.535 m
    return [("32F default", dict(fmt=dn.FMT_32F), False, False),
            ("32F window + conf", dict(fmt=dn.FMT_32F, unit=2.0, z_min=zlo, z_max=zhi, min_conf=0.2), True, True),
            ("32F conf only", dict(fmt=dn.FMT_32F, min_conf=0.4), True, True),
            ("16U unit", dict(fmt=dn.FMT_16U, unit=unit), False, True),
            ("16U window + conf", dict(fmt=dn.FMT_16U, unit=unit / 2, z_min=zlo, z_max=zhi, min_conf=0.1), True, True)]


# ---- 1: a single window -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [(0, 0), (13, -9), CORNER])
def test_single_window_equals_the_composition_and_the_restatement(lib, fctx, orc, off):
    fw, fh, ox, oy, _, _ = orc.fovea_geometry(FW, FH, FLV, FF, *off)
    w, h = orc.level_dims(FW, FH, FLV)
    if off == CORNER:
        assert all(ox[l] == w[l] - fw and oy[l] == h[l] - fh for l in range(FF - 1)), "the window is not against the corner"
    st = make_stack(lib, FW, FH, FLV, FF, off[0])
    field = field_of(orc, [st], FW, FH, FLV, [off])
    for label, kw, conf, both in filtered(orc, field):
        size = 2 if kw["fmt"] == dn.FMT_16U else 4
        check_three_ways(fctx, lib, orc, [st], [off], FW, FH, FLV, params_of(lib, kw), kw, f"{label} off {off}", conf=conf, both=both,
                         shifts=((0, 0), (1, size)), field=field)


# ---- 2: odd shapes and bases ----------------------------------------------------------------------------------------------------------

def test_odd_frame_at_unaligned_bases_touches_nothing_else(lib, octx, orc):
    assert OW % 2 == 1 and (OW * OH) % 8 != 0
    off = (3, -2)
    st = make_stack(lib, OW, OH, OLV, OF, 5)
    field = field_of(orc, [st], OW, OH, OLV, [off])
    cases = filtered(orc, field)
    for label, kw, conf, both in (cases[0], cases[1], cases[3], cases[4]):
        u16 = kw["fmt"] == dn.FMT_16U
        shifts = [(1, 2), (3, 6), (1, 14)] if u16 else [(3, 4), (1, 8), (3, 12)]
        check_three_ways(octx, lib, orc, [st], [off], OW, OH, OLV, params_of(lib, kw), kw, f"{OW}x{OH} {label}", conf=conf, both=both, shifts=shifts,
                         field=field)
    sts = [make_stack(lib, OW, OH, OLV, OF, 6 + j) for j in range(2)]
    kw = dict(fmt=dn.FMT_16U, unit=cases[3][1]["unit"], min_conf=0.1)
    check_three_ways(octx, lib, orc, sts, [(3, -2), (-4, 1)], OW, OH, OLV, params_of(lib, kw), kw, f"{OW}x{OH} two windows 16U",
                     shifts=[(1, 2), (3, 14)])


# ---- 3: wild values -------------------------------------------------------------------------------------------------------------------

def test_wild_values_appear_only_where_nothing_finer_covers_them(lib, fctx, orc):
    """NaN, +-inf, +-3e38 and +-1e-40 in dx and in the confidence at one pixel each of every level: in the middle of the level, which the
    finer level's window covers (levels 1 .. F-1) -- the reconstruction must not change --, and in the level's last row, which nothing
    covers -- they reach the field scaled by s per level descended.  Fused == composition == restatement."""
    off = (0, 0)
    clean = make_stack(lib, FW, FH, FLV, FF, 77, nan_conf=0)
    fw, fh = clean.shape[3], clean.shape[2]
    covered, both = clean.copy(), clean.copy()
    for l in range(FF):
        for i, v in enumerate(WILD):
            if l > 0:
                for st in (covered, both):
                    st[0, l, fh // 2, fw // 2 - 7 + i] = v
                    st[2, l, fh // 2 + 1, fw // 2 - 7 + i] = v
            both[0, l, fh - 1, i] = v
            both[2, l, fh - 1, 7 + i] = v
    f0, fc, fb = (field_of(orc, [st], FW, FH, FLV, [off]) for st in (clean, covered, both))
    assert np.array_equal(fc.view(np.uint32), f0.view(np.uint32)), "a value under a finer window reached the field"
    changed = fb.view(np.uint32) != f0.view(np.uint32)
    assert changed[0].sum() >= 7 * FF and changed[2].sum() >= 7 * FF
    assert np.isnan(fb[0]).sum() > np.isnan(f0[0]).sum() and np.isinf(fb[0]).any() and np.isinf(fb[2]).any()
    tiny = np.float32(1e-40)
    assert (fb[0] == tiny).any() and (fb[0] == S * (S * (S * tiny))).any(), "a denormal of level F-1 reaches the field times s three times"
    for label, kw, conf, _ in filtered(orc, f0)[:1] + filtered(orc, f0)[2:]:
        check_three_ways(fctx, lib, orc, [both], [off], FW, FH, FLV, params_of(lib, kw), kw, f"wild {label}", conf=conf, shifts=((1, 0),), field=fb)


# ---- 4: several windows ---------------------------------------------------------------------------------------------------------------

OFF3 = [(0, 0), (6, 4), (-5, 3)]                                          # overlap at every level
OFF16 = [(-40 + 27 * (j % 4), -30 + 20 * (j // 4)) for j in range(16)]    # scattered, neighbours overlapping


@pytest.fixture(scope="module")
def stacks16(lib):
    return [make_stack(lib, FW, FH, FLV, FF, 200 + j) for j in range(16)]


def test_one_window_through_the_multi_call_is_the_single_call(lib, fctx, orc, stacks16):
    st, off = stacks16[0], (13, -9)
    for kw in (dict(fmt=dn.FMT_32F, min_conf=0.3), dict(fmt=dn.FMT_16U, unit=0.004)):
        prm = params_of(lib, kw)
        one, n1 = fused(fctx, lib, [st], [off], FW, FH, P1, P2, prm, multi=False, in_shift=1)
        many, nm = fused(fctx, lib, [st], [off], FW, FH, P1, P2, prm, multi=True, in_shift=3, out_shift=prm.format * 2 + 4)
        dn.assert_image_equal(many, one, f"n = 1 {kw}")
        assert nm == n1


@pytest.mark.parametrize("n", [3, 16])
def test_several_windows_highest_index_wins(lib, fctx, orc, stacks16, n):
    """n = 3: windows that overlap at every level; n = 16: the table in device memory."""
    offs = OFF3 if n == 3 else OFF16
    sts = stacks16[:n]
    geo = [orc.fovea_geometry(FW, FH, FLV, FF, *o) for o in offs]
    fw, fh = geo[0][0], geo[0][1]
    if n == 3:
        for l in range(FF - 1):
            for a in range(n):
                for b in range(a + 1, n):
                    assert abs(geo[a][2][l] - geo[b][2][l]) < fw and abs(geo[a][3][l] - geo[b][3][l]) < fh, "the windows do not overlap"
    field = field_of(orc, sts, FW, FH, FLV, offs)
    # where the last window lies at level 0 the field is its level 0, whatever lies under it
    ox, oy = geo[-1][2][0], geo[-1][3][0]
    assert np.array_equal(field[:, oy:oy + fh, ox:ox + fw].view(np.uint32), sts[-1][:, 0].view(np.uint32))
    cases = filtered(orc, field)
    for label, kw, _, both in (cases[2], cases[4]):
        check_three_ways(fctx, lib, orc, sts, offs, FW, FH, FLV, params_of(lib, kw), kw, f"n = {n} {label}", both=both,
                         shifts=((1, 2 if kw["fmt"] == dn.FMT_16U else 4),), field=field)


# ---- 5: resized -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("factor", [0.2, 0.5])
def test_resized_images(lib, fctx, orc, stacks16, factor):
    for sts, offs in (([stacks16[4]], [(13, -9)]), (stacks16[:3], OFF3)):
        field = field_of(orc, sts, FW, FH, FLV, offs)
        cases = filtered(orc, field)
        for label, kw, _, _ in (cases[2], cases[4]):
            size = 2 if kw["fmt"] == dn.FMT_16U else 4
            check_three_ways(fctx, lib, orc, sts, offs, FW, FH, FLV, params_of(lib, kw, factor), kw, f"factor {factor} n = {len(sts)} {label}",
                             shifts=((0, 0), (3, size)), field=field)
    st = stacks16[4]
    kw = dict(fmt=dn.FMT_32F)
    check_three_ways(fctx, lib, orc, [st], [(0, 0)], FW, FH, FLV, params_of(lib, kw, factor), kw, f"factor {factor} no confidence", conf=False)


# ---- 6: lens --------------------------------------------------------------------------------------------------------------------------

def test_lens_is_honoured_as_the_composition_honours_it(lib, fctx, orc, stacks16):
    rig = ln.rigs()["small"]
    Q1, Q2 = rig["P1"], rig["P2"]
    zero = (rig["K1"], np.zeros(5), rig["K2"], np.zeros(5), 5)
    for sts, offs in (([stacks16[5]], [(13, -9)]), (stacks16[:3], OFF3)):
        field = field_of(orc, sts, FW, FH, FLV, offs)
        z = orc.triangulate(field[0], field[1], Q1, Q2)[2]
        unit = 60.0 / float(np.percentile(np.abs(z[np.isfinite(z) & (z != 0)]), 80))
        for kw, factor in ((dict(fmt=dn.FMT_32F), 1.0), (dict(fmt=dn.FMT_16U, unit=unit, min_conf=0.1), 1.0), (dict(fmt=dn.FMT_32F, min_conf=0.2), 0.5)):
            prm = params_of(lib, kw, factor)
            what = f"lens n = {len(sts)} {kw} factor {factor}"
            plain, n0 = fused(fctx, lib, sts, offs, FW, FH, Q1, Q2, prm, in_shift=1)
            try:
                fctx.set_lens(*ln.lens_of(rig))
                want, nw = composed(fctx, lib, sts, offs, FW, FH, Q1, Q2, prm)
                got, n = fused(fctx, lib, sts, offs, FW, FH, Q1, Q2, prm, in_shift=1, out_shift=4)
                fctx.set_lens(*zero)
                flat, nz = fused(fctx, lib, sts, offs, FW, FH, Q1, Q2, prm, in_shift=3)
            finally:
                fctx.clear_lens()
            dn.assert_image_equal(got, want, what + ": fused vs the composition under the lens")
            assert n == nw
            assert not np.array_equal(dn.image_bits(got), dn.image_bits(plain)), what + ": the lens changed nothing"
            dn.assert_image_equal(flat, plain, what + ": a zero-D lens vs no lens")
            assert nz == n0


# ---- 7: more than one pass of the grid ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,fmt", [(2049, 1031, dn.FMT_32F), (2049, 1031, dn.FMT_16U), (2049, 2057, dn.FMT_16U)])
def test_images_larger_than_one_pass_of_the_grid(lib, W, H, fmt):
    """A depth launch holds at most 2048 workgroups of 256 runs: 2049 x 1031 has 528 k runs of four 32F pixels, 2049 x 2057 has 527 k runs of
    eight 16U pixels -- the last runs come in a workgroup's second pass.  levels 5, fovea levels 3.  The image equals the composition."""
    levels, F = 5, 3
    st = make_stack(lib, W, H, levels, F, 9)
    kw = dict(fmt=fmt, unit=0.004 if fmt == dn.FMT_16U else 1.0, min_conf=0.1)
    with lib.Context(levels=levels, fovea_levels=F) as c:
        prm = params_of(lib, kw)
        want, nw = composed(c, lib, [st], [(40, -25)], W, H, P1, P2, prm)
        got, n = fused(c, lib, [st], [(40, -25)], W, H, P1, P2, prm, in_shift=1, out_shift=2 if fmt == dn.FMT_16U else 4)
    dn.assert_image_equal(got, want, f"{W}x{H} format {fmt}")
    assert n == nw and 0 < n < W * H


# ---- 8: the blocking call -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mono", [False, True])
def test_match_foveated_depth_is_match_foveated_then_the_fused_call(lib, orc, mono):
    from ug_stereomatcher_amd import synth
    P2M = P1.copy()          # the rig mirrored: the synthetic pairs' disparities are positive
    P2M[0, 3] = 7.3230899280915291e+03 * 0.12
    W, H, levels, F, off = 64, 48, 5, 2, (5, -3)
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 7)
    if mono:
        L, R = np.ascontiguousarray(L[..., 1]), np.ascontiguousarray(R[..., 1])
    with lib.Context(levels=levels, fovea_levels=F) as c:
        if mono:
            c.set_input_format(lib.UGSM_INPUT_MONO8)
        fw, fh = lib.fovea_dims(W, H, levels, F)
        st = np.empty((3, F, fh, fw), np.float32)
        c.check(c.lib.ugsm_match_foveated(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], off[0], off[1],
                                          *(st[k].ctypes.data for k in range(3)), None, None))
        field = field_of(orc, [st], W, H, levels, [off])
        z = orc.triangulate(field[0], field[1], P1, P2M)[2]
        unit = 60.0 / float(np.percentile(z[np.isfinite(z) & (z > 0)], 80))
        for kw, factor in ((dict(fmt=dn.FMT_32F), 1.0), (dict(fmt=dn.FMT_16U, unit=unit, min_conf=0.05), 1.0), (dict(fmt=dn.FMT_32F, min_conf=0.05), 0.5)):
            prm = params_of(lib, kw, factor)
            want, _ = fused(c, lib, [st], [off], W, H, P1, P2M, prm, what=f"the fused call on the stack {kw}")
            exp, _ = restated(orc, field, P1, P2M, factor=factor, **kw)
            dn.assert_image_equal(want, exp, f"the fused call vs the restatement {kw}")
            alone = c.match_foveated_depth(L, R, P1, P2M, prm, off=off)
            dn.assert_image_equal(alone, want, f"ugsm_match_foveated_depth, no stack, mono={mono} {kw}")
            both, out = c.match_foveated_depth(L, R, P1, P2M, prm, off=off, stack=True)
            dn.assert_image_equal(both, want, f"ugsm_match_foveated_depth, with the stack, mono={mono} {kw}")
            assert np.array_equal(out.view(np.uint32), st.view(np.uint32))
        # one plane alone comes down where only it is asked for
        depth, only = np.empty((H, W), np.float32), np.full((F, fh, fw), -1.0, np.float32)
        P = [(C.c_double * 12)(*np.asarray(p, np.float64).reshape(12)) for p in (P1, P2M)]
        c.check(c.lib.ugsm_match_foveated_depth(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], off[0], off[1], P[0], P[1],
                                                C.byref(lib.depth_params()), depth.ctypes.data, None, None, only.ctypes.data))
        assert np.array_equal(only.view(np.uint32), st[2].view(np.uint32))
        want16 = c.match_foveated_depth(L, R, P1, P2M, lib.depth_params(format=lib.UGSM_DEPTH_16U, unit=unit), off=off)
    if mono:
        return
    from ug_stereomatcher_amd import MatchGPULib
    m = MatchGPULib(3, ["node", "x", str(F)], levels=levels)
    try:
        got16, stack = m.depthImageFrame(L, R, P1, P2M, "16UC1", unit=unit, off_x=off[0], off_y=off[1], stack=True)
        dn.assert_image_equal(got16, want16, "MatchGPULib.depthImageFrame 16UC1")
        assert np.array_equal(stack.view(np.uint32), np.transpose(st, (1, 0, 2, 3)).view(np.uint32))
        with pytest.raises(lib.UgsmError):
            m.depthImageFrame(L, R, P1, P2M, "8UC1")
    finally:
        m.close()


# ---- 9: the refusals on a live context --------------------------------------------------------------------------------------------------

from test_depth_frame_host import CALLS, bad_argument_cases, call, resolve  # noqa: E402


def _live_buffers(c, lib, W, H, levels, F, n=3):
    fw, fh = lib.fovea_dims(W, H, levels, F)
    plane = F * fw * fh
    host = np.concatenate([np.full(plane, -30.0, np.float32), np.zeros(plane, np.float32), np.ones(plane, np.float32)])   # (a finite Z everywhere)
    stacks = [c.to_device(host) for _ in range(n)]
    bufs = dict(dx=stacks[0], dy=stacks[0] + 4 * plane, conf=stacks[0] + 8 * plane, stack1=stacks[1], stack2=stacks[2],
                depth=c.to_device(np.full(W * H * 4, POISON, np.uint8)), valid=c.to_device(np.full(1, 0xDEADBEEF, np.uint64)))
    return stacks, bufs


def test_refusals_on_a_live_context_write_nothing_and_name_the_call(lib, fctx):
    stacks, bufs = _live_buffers(fctx, lib, FW, FH, FLV, FF)
    L = np.zeros((FH, FW, 3), np.uint8)
    host = np.full(FW * FH, -3.0, np.float32)

    def untouched():
        fctx.check(fctx.lib.ugsm_wait(fctx.handle, 0))
        return ((fctx.to_host(bufs["depth"], (FW * FH * 4,), np.uint8) == POISON).all()
                and fctx.to_host(bufs["valid"], (1,), np.uint64)[0] == 0xDEADBEEF and (host == -3.0).all())
    try:
        for name in CALLS:
            live = dict(bufs, ctx=fctx.handle, W=FW, H=FH, stacks=stacks)
            if name == "ugsm_match_foveated_depth":
                live.update(L=L.ctypes.data, R=L.ctypes.data, stride=3 * FW, depth=host.ctypes.data)
            for label, over in bad_argument_cases(lib, name):
                a = dict(live)
                a.update(resolve(over, bufs))
                assert call(lib, name, **a) == lib.UGSM_ERR_BAD_ARG, (name, label)
                assert name.encode() in fctx.lib.ugsm_last_error(fctx.handle), (name, label, fctx.lib.ugsm_last_error(fctx.handle))
            assert untouched(), name
        with lib.Context(levels=5, fovea_levels=1) as c1:     # a stack has at least two levels
            for name in CALLS[:2]:
                assert call(lib, name, **dict(bufs, ctx=c1.handle, W=FW, H=FH, stacks=stacks)) == lib.UGSM_ERR_BAD_ARG
                assert name.encode() in c1.lib.ugsm_last_error(c1.handle)
        assert untouched()
        rig = dict(P1=(C.c_double * 12)(*P1.reshape(12)), P2=(C.c_double * 12)(*P2.reshape(12)))
        for name in CALLS[:2]:
            assert call(lib, name, **dict(bufs, ctx=fctx.handle, W=FW, H=FH, stacks=stacks, **rig)) == lib.UGSM_OK
            fctx.check(fctx.lib.ugsm_wait(fctx.handle, 0))
            assert fctx.to_host(bufs["valid"], (1,), np.uint64)[0] == FW * FH
    finally:
        for p in stacks + [bufs["depth"], bufs["valid"]]:
            fctx.free(p)


def test_refused_while_enqueued_pairs_are_outstanding(lib):
    from ug_stereomatcher_amd import synth
    L, R, _, _ = synth.make_pair(FW, FH, synth.BASE_SEED + 9)
    rig = dict(P1=(C.c_double * 12)(*P1.reshape(12)), P2=(C.c_double * 12)(*P2.reshape(12)))
    with lib.Context(levels=FLV, fovea_levels=FF, slots=2) as c:
        stacks, bufs = _live_buffers(c, lib, FW, FH, FLV, FF)
        dL, dR, d_out = c.to_device(L), c.to_device(R), c.alloc(3 * FW * FH * 4)
        full = dict(bufs, ctx=c.handle, W=FW, H=FH, stacks=stacks, **rig)
        try:
            c.enqueue_full(dL, dR, FW, FH, L.strides[0], d_out, 7)
            for name in CALLS[:2]:
                assert call(lib, name, **full) == lib.UGSM_ERR_STATE
                err = c.lib.ugsm_last_error(c.handle)
                assert name.encode() in err and b"queue" in err
            done = c.drain()
            assert [int(d.tag) for d in done] == [7] and done[0].status == 0
            assert (c.to_host(bufs["depth"], (FW * FH * 4,), np.uint8) == POISON).all()
            assert c.to_host(bufs["valid"], (1,), np.uint64)[0] == 0xDEADBEEF
            for name in CALLS[:2]:
                assert call(lib, name, **full) == lib.UGSM_OK
                c.check(c.lib.ugsm_wait(c.handle, 0))
                assert c.to_host(bufs["valid"], (1,), np.uint64)[0] == FW * FH
        finally:
            for p in stacks + [bufs["depth"], bufs["valid"], dL, dR, d_out]:
                c.free(p)


# ---- 10: memory -----------------------------------------------------------------------------------------------------------------------

def test_the_fused_call_grows_the_slot_by_a_table_never_by_a_field(lib):
    """ugsm_context_device_bytes across the first fused calls of a fresh context: nothing for one window, the same table for three at
    160 x 120 and at 640 x 480; the composition on a fresh context at 640 x 480 grows it by level buffers."""
    rig = dict(P1=(C.c_double * 12)(*P1.reshape(12)), P2=(C.c_double * 12)(*P2.reshape(12)))
    growth = {}
    for W, H in ((FW, FH), (640, 480)):
        with lib.Context(levels=FLV, fovea_levels=FF) as c:
            stacks, bufs = _live_buffers(c, lib, W, H, FLV, FF)
            try:
                b0 = c.device_bytes()
                assert call(lib, CALLS[0], **dict(bufs, ctx=c.handle, W=W, H=H, stacks=stacks, **rig)) == lib.UGSM_OK
                c.check(c.lib.ugsm_wait(c.handle, 0))
                b1 = c.device_bytes()
                assert call(lib, CALLS[1], **dict(bufs, ctx=c.handle, W=W, H=H, stacks=stacks, **rig)) == lib.UGSM_OK
                c.check(c.lib.ugsm_wait(c.handle, 0))
                growth[W] = (b1 - b0, c.device_bytes() - b1)
                assert c.to_host(bufs["valid"], (1,), np.uint64)[0] == W * H
            finally:
                for p in stacks + [bufs["depth"], bufs["valid"]]:
                    c.free(p)
    assert growth[FW] == growth[640], growth
    assert growth[FW][0] == 0 and 0 < growth[FW][1] < 64 * 1024, growth
    W, H = 640, 480
    with lib.Context(levels=FLV, fovea_levels=FF) as c:
        stacks, bufs = _live_buffers(c, lib, W, H, FLV, FF)
        d_field = c.alloc(3 * W * H * 4)
        try:
            b0 = c.device_bytes()
            c.reconstruct_full(bufs["dx"], bufs["dy"], bufs["conf"], W, H, d_field)
            c.depth_image(d_field, d_field + 4 * W * H, d_field + 8 * W * H, W, H, P1, P2, lib.depth_params(), bufs["depth"], bufs["valid"])
            composition = c.device_bytes() - b0
        finally:
            for p in stacks + [bufs["depth"], bufs["valid"], d_field]:
                c.free(p)
    w, h = lib.level_dims(W, H, FLV)
    assert composition >= 3 * w[1] * h[1] * 4 > sum(growth[640]), (composition, growth)      # (ensure_level_bufs: 3 w[1] h[1] floats a buffer)
