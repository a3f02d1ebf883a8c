"""The warped right image and the photometric residual of a match on the device (ugsm_warp_planes, ugsm_warp_right,
ugsm_warp_right_fovea, ugsm_photometric_residual, ugsm_photometric_residual_fovea): bit for bit against the fixture written from the
reference's own `warp` stage (tests/golden/warp_right.npz), the numpy restatement (tests/warp_np.py) and the oracle's weightedDifference."""
import ctypes as C

import numpy as np
import pytest

import encode_np as en
import warp_np as wn
from conftest import assert_bit_equal, load_golden
from test_warp_host import NEW, bad_argument_cases

pytestmark = pytest.mark.gpu

LEVELS = 8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(levels=LEVELS, fovea_levels=4, slots=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return load_golden("warp_right.npz")


@pytest.fixture(scope="module")
def cases():
    """Per shape: the fixture's inputs and the warped right planes by the restatement (computed once, shared, never written to)."""
    out = []
    for k in range(len(wn.SHAPES)):
        L, R, d, wild = wn.fixture_inputs(k)
        out.append(dict(L=L, R=R, d=d, wild=wild, Rw=wn.warp(wn.planes(R), d[0], d[1])))
    return out


class Dev:
    """Device buffers of one test, freed together; images may be laid out with padded rows and at an odd address."""

    def __init__(self, c):
        self.c, self.bufs = c, []

    def image(self, img, pad=0, shift=0):
        rows = en.padded(img, pad)
        base = self.c.alloc(rows.nbytes + 64)
        self.bufs.append(base)
        raw = np.zeros(rows.nbytes + 64, np.uint8)
        raw[shift:shift + rows.nbytes] = rows.reshape(-1)
        self.c.check(self.c.lib.ugsm_copy_to_device(self.c.handle, base, raw.ctypes.data, raw.nbytes))
        return base + shift, rows.shape[1]

    def put(self, arr):
        p = self.c.to_device(np.ascontiguousarray(arr))
        self.bufs.append(p)
        return p

    def out(self, nfloats):
        return self.put(np.full(nfloats, np.nan, np.float32))

    def free(self):
        for p in self.bufs:
            self.c.free(p)
        self.bufs = []


def _wd(orc, L3, Rw3, conf):
    """float32(S_c / C) for the three channels by the oracle's weighted_difference"""
    c = np.ones(L3.shape[1:], np.float32) if conf is None else conf
    a = orc.weighted_difference(np.stack([L3[0], L3[1], c]), np.stack([Rw3[0], Rw3[1], c]))
    b = orc.weighted_difference(np.stack([L3[2], L3[1], c]), np.stack([Rw3[2], Rw3[1], c]))
    return np.array([a[0], a[1], b[0]], np.float32)


# ---- 1. the warp against the fixture ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(wn.SHAPES)))
def test_warp_right_and_warp_planes_equal_the_fixture(ctx, golden, cases, k):
    W, H = wn.SHAPES[k]
    cs = cases[k]
    ctx.set_input_format(en.RGB8)
    d = Dev(ctx)
    try:
        img, stride = d.image(cs["R"], pad=5, shift=1)          # stride 3 W + 5, the image at an odd address
        assert stride > 3 * W and img % 2 == 1
        five = np.concatenate([wn.planes(cs["R"]), wn.planes(cs["L"])[:2]])
        src = d.put(five)
        for name, f in (("", cs["d"]), ("_wild", cs["wild"])):
            if f is None:
                continue
            want = golden[f"{W}x{H}{name}"].astype(np.float32)
            dx, dy = d.put(f[0]), d.put(f[1])
            o = d.out(3 * W * H)
            ctx.warp_right(img, W, H, stride, dx, dy, o)
            assert_bit_equal(ctx.to_host(o, (3, H, W)), want, f"ugsm_warp_right vs the fixture, {W}x{H}{name}")
            for channels in (1, 3, 5):
                o = d.out(5 * W * H)
                ctx.warp_planes(src, channels, W, H, dx, dy, o)
                got = ctx.to_host(o, (5, H, W))
                assert_bit_equal(got[:min(channels, 3)], want[:min(channels, 3)], f"ugsm_warp_planes vs the fixture, {W}x{H}{name}, {channels} planes")
                assert_bit_equal(got[:channels], wn.warp(five[:channels], f[0], f[1]), f"ugsm_warp_planes vs warp_np, {channels} planes")
                assert np.isnan(got[channels:]).all(), "planes past `channels` were written"
    finally:
        d.free()


# ---- 2. the five input formats ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", en.FORMATS)
def test_input_formats_equal_their_rgb8_conversion(ctx, cases, fmt):
    k = wn.SHAPES.index((130, 75))
    W, H = wn.SHAPES[k]
    cs = cases[k]
    encL, encR = en.encode(cs["L"], fmt), en.encode(cs["R"], fmt)
    rgbL, rgbR = en.to_rgb8(encL, fmt), en.to_rgb8(encR, fmt)
    layouts = [(0, 0), (8, 0)] + ([(8, 1)] if en.BPP[fmt] == 4 else [])   # the four-byte formats: word loads, and byte loads when misaligned
    d = Dev(ctx)
    try:
        dx, dy, conf = (d.put(p) for p in cs["d"])
        ctx.set_input_format(en.RGB8)
        (pl, sl), (pr, sr) = d.image(rgbL), d.image(rgbR)
        o = d.out(3 * W * H)
        ctx.warp_right(pr, W, H, sr, dx, dy, o)
        want = ctx.to_host(o, (3, H, W))
        assert_bit_equal(want, wn.warp(wn.planes(rgbR), cs["d"][0], cs["d"][1]), "the rgb8 conversion vs warp_np")
        ctx.photometric_residual(pl, pr, W, H, sl, dx, dy, conf)
        want_sums = ctx.last_residual_sums.tobytes()
        for pad, shift in layouts:
            ctx.set_input_format(fmt)
            (pl, sl), (pr, sr) = d.image(encL, pad, shift), d.image(encR, pad, shift)
            o = d.out(3 * W * H)
            ctx.warp_right(pr, W, H, sr, dx, dy, o)
            got = ctx.to_host(o, (3, H, W))
            assert_bit_equal(got, want, f"ugsm_warp_right in {en.NAMES[fmt]} (pad {pad}, shift {shift}) vs its rgb8 conversion")
            if fmt == en.MONO8:
                assert_bit_equal(got[1], got[0], "mono8: plane 1")
                assert_bit_equal(got[2], got[0], "mono8: plane 2")
            ctx.photometric_residual(pl, pr, W, H, sl, dx, dy, conf)
            assert ctx.last_residual_sums.tobytes() == want_sums, f"the residual in {en.NAMES[fmt]} (pad {pad}, shift {shift})"
    finally:
        ctx.set_input_format(en.RGB8)
        d.free()


# ---- 3. the stack forms -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,levels,F,fov", [(320, 240, 9, 4, (112, 84)), (333, 251, 8, 3, None)])
def test_fovea_stack_forms(lib, orc, W, H, levels, F, fov):
    from ug_stereomatcher_amd import synth
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 71)
    stack, pl, pr = orc.match_foveated(L, R, levels, F, want_pyr=True)
    fw, fh = lib.fovea_dims(W, H, levels, F)
    assert stack.shape == (3, F, fh, fw) and pl.shape == (F, 3, fh, fw)
    if fov:
        assert (fw, fh) == fov and fh > 64
    n = fw * fh
    warped = [wn.warp(pr[k], stack[0, k], stack[1, k]) for k in range(F)]
    with lib.Context(levels=levels, fovea_levels=F) as c:
        d = Dev(c)
        dS, dL, dR = d.put(stack), d.put(pl), d.put(pr)
        dW = d.out(F * 3 * n)
        c.warp_right_fovea(dR, dS, dS + 4 * F * n, fw, fh, dW)
        got = c.to_host(dW, (F, 3, fh, fw))
        for k in range(F):
            assert_bit_equal(got[k], warped[k], f"ugsm_warp_right_fovea, level {k}")
        for conf in (stack[2], None):
            q, total = c.photometric_residual_fovea(dL, dR, dS, dS + 4 * F * n, dS + 8 * F * n if conf is not None else None, fw, fh)
            raw = c.last_residual_sums
            assert raw.shape == (F, 4) and q.shape == (F, 3)
            for k in range(F):
                ck = None if conf is None else conf[k]
                assert raw[k].tobytes() == wn.residual_sums(pl[k], warped[k], ck).tobytes(), f"the raw sums of level {k}: {raw[k]}"
                assert_bit_equal(q[k], _wd(orc, pl[k], warped[k], ck), f"S / C of level {k} vs weighted_difference")
                assert total[k] == raw[k, 3]
        d.free()


# ---- 4. the residual of a full-resolution field -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(wn.SHAPES)))
def test_photometric_residual(ctx, orc, cases, k):
    W, H = wn.SHAPES[k]
    cs = cases[k]
    L3 = wn.planes(cs["L"])
    ctx.set_input_format(en.RGB8)
    d = Dev(ctx)
    try:
        (pl, stride), (pr, _) = d.image(cs["L"], pad=5, shift=1), d.image(cs["R"], pad=5, shift=1)
        dx, dy, dc = (d.put(p) for p in cs["d"])
        dw = d.out(3 * W * H)
        ctx.warp_right(pr, W, H, stride, dx, dy, dw)
        written = ctx.to_host(dw, (3, H, W))
        for conf, dconf in ((cs["d"][2], dc), (None, None)):
            q, total = ctx.photometric_residual(pl, pr, W, H, stride, dx, dy, dconf)
            raw = ctx.last_residual_sums[0].copy()
            want = wn.residual_sums(L3, cs["Rw"], conf)
            print(f"{W}x{H} conf={'field' if conf is not None else 'NULL'}: sums {raw.tolist()} S/C {q.tolist()}")
            assert raw.tobytes() == want.tobytes(), f"the raw sums: {raw} vs {want}"
            assert total == want[3]
            assert_bit_equal(q, _wd(orc, L3, cs["Rw"], conf), "S / C vs weighted_difference")
            # the same number from the planes ugsm_warp_right wrote, through row f-4's own kernels
            c = np.ones((H, W), np.float32) if conf is None else conf
            out2 = (C.c_float * 2)()
            for a, b, chans in ((0, 1, (0, 1)), (2, 1, (2, 1))):
                new3 = d.put(np.stack([L3[a], L3[b], c]))
                old3 = d.put(np.stack([written[a], written[b], written[a]]))
                ctx.check(ctx.lib.ugsm_stage_weighted_difference(ctx.handle, new3, old3, W, H, out2))
                assert_bit_equal(np.array(out2[:], np.float32), q[list(chans)], f"ugsm_stage_weighted_difference on the warped planes, channels {chans}")
            q2, _ = ctx.photometric_residual(pl, pr, W, H, stride, dx, dy, dconf)
            assert ctx.last_residual_sums[0].tobytes() == raw.tobytes() and q2.tobytes() == q.tobytes(), "two runs differ"
    finally:
        d.free()


# ---- 5. meaning -----------------------------------------------------------------------------------------------------------------------------

def test_the_matched_field_lowers_the_residual(ctx):
    from ug_stereomatcher_amd import synth
    W, H = 160, 120
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 101)
    ctx.set_input_format(en.RGB8)
    d = Dev(ctx)
    try:
        dL, dR = d.put(L), d.put(R)
        o = d.out(3 * W * H)
        zero = d.put(np.zeros((H, W), np.float32))
        ctx.check(ctx.lib.ugsm_submit_full(ctx.handle, 0, dL, dR, W, H, 3 * W, o))
        matched, _ = ctx.photometric_residual(dL, dR, W, H, 3 * W, o, o + 4 * W * H, o + 8 * W * H)   # (right behind the submit: same slot)
        unmoved, _ = ctx.photometric_residual(dL, dR, W, H, 3 * W, zero, zero, o + 8 * W * H)
        print("matched", matched.tolist(), "unmoved", unmoved.tolist())
        assert (matched < unmoved).all(), (matched, unmoved)
    finally:
        d.free()


# ---- 6. ordering and refusals ---------------------------------------------------------------------------------------------------------------

def test_a_call_right_behind_a_submit_is_ordered_behind_it(ctx):
    from ug_stereomatcher_amd import synth
    W, H = 160, 120
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 101)
    ctx.set_input_format(en.RGB8)
    d = Dev(ctx)
    try:
        dL, dR = d.put(L), d.put(R)
        o, w1, w2 = d.out(3 * W * H), d.out(3 * W * H), d.out(3 * W * H)
        ctx.check(ctx.lib.ugsm_submit_full(ctx.handle, 1, dL, dR, W, H, 3 * W, o))
        ctx.warp_right(dR, W, H, 3 * W, o, o + 4 * W * H, w1, slot=1, wait=False)     # no wait in between
        ctx.check(ctx.lib.ugsm_wait(ctx.handle, 1))
        ctx.warp_right(dR, W, H, 3 * W, o, o + 4 * W * H, w2, slot=1)
        field = ctx.to_host(o, (3, H, W))
        first = ctx.to_host(w1, (3, H, W))
        assert_bit_equal(first, ctx.to_host(w2, (3, H, W)), "behind the submit without a wait vs after a wait")
        assert_bit_equal(first, wn.warp(wn.planes(R), field[0], field[1]), "the warp by the matched field vs warp_np")
    finally:
        d.free()


def _real(c, lib, name, b, **over):
    """One call of `name` on a live context with real device buffers of b (every one large enough for any accepted call at 64 x 48)."""
    a = dict(slot=0, src=b["a"], L=b["a"], R=b["b"], dx=b["dx"], dy=b["dy"], conf=b["conf"], dst=b["dst"], sums=b["sums"], W=64, H=48,
             channels=3)
    a.update({k: (b[v] if isinstance(v, str) else v) for k, v in over.items()})
    if "sums" in over and over["sums"] is not None:
        a["sums"] = b["sums"] + 4                                # (the misaligned case)
    stride = a.get("stride", 3 * max(a["W"], 1))
    so = c.lib
    if name == "ugsm_warp_planes":
        return so.ugsm_warp_planes(c.handle, a["slot"], a["src"], a["channels"], a["W"], a["H"], a["dx"], a["dy"], a["dst"])
    if name == "ugsm_warp_right":
        return so.ugsm_warp_right(c.handle, a["slot"], a["R"], a["W"], a["H"], stride, a["dx"], a["dy"], a["dst"])
    if name == "ugsm_warp_right_fovea":
        return so.ugsm_warp_right_fovea(c.handle, a["slot"], a["R"], a["dx"], a["dy"], a["W"], a["H"], a["dst"])
    if name == "ugsm_photometric_residual":
        return so.ugsm_photometric_residual(c.handle, a["slot"], a["L"], a["R"], a["W"], a["H"], stride, a["dx"], a["dy"], a["conf"], a["sums"])
    return so.ugsm_photometric_residual_fovea(c.handle, a["slot"], a["L"], a["R"], a["dx"], a["dy"], a["conf"], a["W"], a["H"], a["sums"])


def test_refusals_state_and_scratch(lib):
    from ug_stereomatcher_amd import synth
    W, H, F = 64, 48, 4
    n = W * H
    L, R, _, _ = synth.make_pair(160, 120, synth.BASE_SEED + 101)
    with lib.Context(levels=LEVELS, fovea_levels=F, slots=2) as c:
        d = Dev(c)
        zeros = np.zeros(3 * F * n, np.float32)
        b = {key: d.put(zeros) for key in ("a", "b", "dx", "dy", "conf", "dst")}
        b["sums"] = d.put(np.zeros(64, np.float64))
        held = c.lib.ugsm_context_device_bytes(c.handle)
        for name in NEW:
            for label, over in bad_argument_cases(name):
                over = {k: ("a" if (k, v) == ("dst", 0x10000) else "b" if (k, v) == ("dst", 0x20000) else v) for k, v in over.items()}
                assert _real(c, lib, name, b, **over) == lib.UGSM_ERR_BAD_ARG, (name, label)
        assert c.lib.ugsm_context_device_bytes(c.handle) == held, "a refused call allocated"
        # the scratch: 4 doubles per row (and level), once
        assert _real(c, lib, "ugsm_photometric_residual", b) == lib.UGSM_OK
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert c.lib.ugsm_context_device_bytes(c.handle) == held + 4 * 8 * H
        assert _real(c, lib, "ugsm_photometric_residual", b, conf=None) == lib.UGSM_OK
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert c.lib.ugsm_context_device_bytes(c.handle) == held + 4 * 8 * H, "the scratch grew again"
        assert _real(c, lib, "ugsm_photometric_residual_fovea", b) == lib.UGSM_OK
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert c.lib.ugsm_context_device_bytes(c.handle) == held + 4 * 8 * H * F
        for name in NEW:                                          # every form is accepted with these arguments
            assert _real(c, lib, name, b) == lib.UGSM_OK, name
        c.check(c.lib.ugsm_wait(c.handle, 0))
        # a pair outstanding in the queue: the slots are the queue's
        dL, dR = d.put(L), d.put(R)
        out = d.out(3 * 160 * 120)
        c.enqueue_full(dL, dR, 160, 120, 3 * 160, out, 7)
        for name in NEW:
            assert _real(c, lib, name, b) == lib.UGSM_ERR_STATE, name
        done = c.drain()
        assert [int(x.tag) for x in done] == [7] and done[0].status == 0
        for name in NEW:
            assert _real(c, lib, name, b) == lib.UGSM_OK, name
        c.check(c.lib.ugsm_wait(c.handle, 0))
        d.free()
    with lib.Context(levels=LEVELS, fovea_levels=1) as c:         # a context without a fovea
        d = Dev(c)
        zeros = np.zeros(3 * F * n, np.float32)
        b = {key: d.put(zeros) for key in ("a", "b", "dx", "dy", "conf", "dst")}
        b["sums"] = d.put(np.zeros(64, np.float64))
        for name in ("ugsm_warp_right_fovea", "ugsm_photometric_residual_fovea"):
            assert _real(c, lib, name, b) == lib.UGSM_ERR_BAD_ARG, name
        assert _real(c, lib, "ugsm_warp_right", b) == lib.UGSM_OK  # the context still serves calls
        c.check(c.lib.ugsm_wait(c.handle, 0))
        d.free()


# ---- 7. the class surface -------------------------------------------------------------------------------------------------------------------

def test_shim_warp_right_image_equals_warp_planes(ctx, cases, golden):
    from ug_stereomatcher_amd import MatchGPULib
    k = 1
    W, H = wn.SHAPES[k]
    cs = cases[k]
    right = wn.planes(cs["R"])
    m = MatchGPULib(levels=LEVELS)
    try:
        got = m.warpRightImage([p for p in right], [cs["d"][0], cs["d"][1]], 3, W, H)
    finally:
        m.close()
    d = Dev(ctx)
    try:
        src, dx, dy = d.put(right), d.put(cs["d"][0]), d.put(cs["d"][1])
        o = d.out(3 * W * H)
        ctx.warp_planes(src, 3, W, H, dx, dy, o)
        assert_bit_equal(got, ctx.to_host(o, (3, H, W)), "MatchGPULib.warpRightImage vs ugsm_warp_planes")
        assert_bit_equal(got, golden[f"{W}x{H}"].astype(np.float32), "MatchGPULib.warpRightImage vs the fixture")
    finally:
        d.free()
