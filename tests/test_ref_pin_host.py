"""The CPU oracle and the numpy restatement against the REFERENCE'S OWN stage code, run on the CPU, bit for bit.

oracle/_ref/libmatchlib_cpu.so is the reference's MatchLib.cu, compiled by g++ from where the checkout lies through the stand-in headers of
oracle/ref_cpu/ (no contraction: the literal contract of DESIGN.md section 3).  Where it was built, every stage function is fed the oracle's own
inputs and its output compared with the matching step of oracle/ugsm_oracle.c and of tests/golden/restate_np.py; where it was not, the live tests
skip and tests/golden/ref_stages.npz -- what that library gave for stored inputs (tests/golden/make_golden.py) -- carries the pin.

What this pins is the ARITHMETIC of every stage.  The order of the calls, the buffers that alias, the taps and the threshold schedule belong to
the host class (MatchGPULib.cpp): tests/ref_stages.py restates them from the cited lines, and a misreading of the host's ordering that oracle,
restatement and that composition share would still pass HERE.  tests/test_ref_driver_host.py closes that: the host class itself, run on the CPU.  Out of scope: weightedDifferenceGPU / reduceGPU (early exit is
off in the reference and the project sums in double on purpose).  NaN texture coordinates are never given to the library.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

import ref_stages as rs
from conftest import GOLDEN, assert_bit_equal, load_golden

sys.path.insert(0, GOLDEN)
import restate_np as rn  # noqa: E402

F32 = np.float32
SHAPES = [(37, 29), (61, 45), (130, 75)]
THIN = [(1, 40), (40, 1)]


@pytest.fixture(scope="module")
def ref(orc):
    r = rs.load(orc)
    if r is None:
        pytest.skip("oracle/_ref/libmatchlib_cpu.so was not built (no reference checkout): tests/golden/ref_stages.npz carries the pin")
    return r


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_stages.npz")


def ran(what, **counts):
    """Every named branch must have run; the counts are printed (pytest -s / -rP) per stage."""
    print(f"{what}: " + ", ".join(f"{k}={int(v)}" for k, v in counts.items()))
    missing = [k for k, v in counts.items() if int(v) == 0]
    assert not missing, f"{what}: no input reached {missing}"


def inputs(W, H):
    L, R = rs.pair(W, H, 7000 + W)
    return rs.planes(L), rs.planes(R), rs.seed_field(W, H, 7100 + H)


# ---- the stand-in's own semantics ------------------------------------------------------------------------------------------------------------

def test_shim_tex2d_point_clamp_unnormalised(ref):
    """tex2D of a never-configured texture reference: texel floor(coordinate), clamped to the array -- below 0, at n - 0.5, at and beyond n,
    +-inf."""
    w, h = 5, 3
    data = np.arange(w * h, dtype=F32).reshape(h, w) + 100
    xs = np.array([-0.5, -3.0, -1e-30, 0.0, 0.999, 1.0, w - 0.5, w - 1e-3, float(w), w + 10.0, 3e38, np.inf, -np.inf, 2.5], F32)
    want_x = np.array([0, 0, 0, 0, 0, 1, w - 1, w - 1, w - 1, w - 1, w - 1, w - 1, 0, 2])
    ys = np.array([-0.5, -7.0, 0.0, 0.5, h - 0.5, float(h), h + 2.0, np.inf, -np.inf], F32)
    want_y = np.array([0, 0, 0, 0, h - 1, h - 1, h - 1, h - 1, 0])
    X, Y = np.meshgrid(xs, ys)
    out = np.empty(X.size, F32)
    f = ref.lib.shim_tex2d
    f.argtypes = [C.c_void_p] + [C.c_int] * 2 + [C.c_void_p] * 3 + [C.c_int]
    x1, y1 = np.ascontiguousarray(X.ravel()), np.ascontiguousarray(Y.ravel())
    f(data.ctypes.data, w, h, x1.ctypes.data, y1.ctypes.data, out.ctypes.data, X.size)
    assert_bit_equal(out.reshape(X.shape), data[want_y[:, None], want_x[None, :]], "tex2D")


def test_shim_min_max_overloads(ref):
    """min / max with float and double mixed: (float, float) stays float, anything with a double is compared and returned in double; a NaN
    loses to the other operand (fmin / fmax)."""
    L = ref.lib
    for name, a, b in (("ff", C.c_float, C.c_float), ("fd", C.c_float, C.c_double), ("df", C.c_double, C.c_float), ("dd", C.c_double, C.c_double)):
        for op in ("min", "max"):
            f = getattr(L, f"shim_{op}_{name}")
            f.argtypes, f.restype = [a, b], (C.c_float if name == "ff" else C.c_double)
    assert (L.shim_sizeof_min_ff(), L.shim_sizeof_min_fd(), L.shim_sizeof_max_df()) == (4, 8, 8)
    tenth_f = float(F32(0.1))  # 0.100000001490116..., above the double 0.1
    assert L.shim_min_fd(0.1, 0.1) == 0.1 and L.shim_max_fd(0.1, 0.1) == tenth_f
    assert L.shim_min_df(0.1, 0.1) == 0.1 and L.shim_max_df(0.1, 0.1) == tenth_f
    assert L.shim_min_ff(2.0, -3.0) == -3.0 and L.shim_max_ff(2.0, -3.0) == 2.0
    nan = float("nan")
    assert L.shim_min_fd(nan, 1.5) == 1.5 and L.shim_max_fd(nan, 1.5) == 1.5 and L.shim_min_fd(1.5, nan) == 1.5
    assert L.shim_max_df(nan, 1.5) == 1.5 and L.shim_min_ff(nan, 1.5) == 1.5 and L.shim_max_ff(1.5, nan) == 1.5
    assert np.isnan(L.shim_min_dd(nan, nan))
    assert L.shim_max_fd(-0.25, 0.0 - 1.0) == -0.25 and L.shim_min_fd(1.0, 7.0) == 1.0  # the parabola's clamp, MatchLib.cu:814
    L.shim_mul24.restype = C.c_int
    assert L.shim_mul24(16, 7) == 112 and L.shim_mul24(-3, 5) == -15 and L.shim_mul24((1 << 24) + 3, 2) == 6


def test_shim_barrier_and_block_order(ref):
    """__syncthreads between real threads, threads that leave early, one block at a time (the static __shared__ array)."""
    gx, gy, bx, by = 3, 2, 16, 8
    n = bx * by
    out = np.full(gx * gy * n, -1, np.int32)
    ref.lib.shim_barrier_probe.argtypes = [C.c_void_p] + [C.c_int] * 4
    ref.lib.shim_barrier_probe(out.ctypes.data, gx, gy, bx, by)
    want = np.concatenate([b * 1000 + (np.arange(n) + 1) % n for b in range(gx * gy)])
    assert (out == want).all()


# ---- stage by stage ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES + THIN)
def test_stage_warp(ref, orc, W, H):
    """warp (MatchLib.cu:499-549) against the oracle's and the restatement's fetch t[clamp(floor(y + dy))][clamp(floor(x + dx))]."""
    pl, pr, d = inputs(W, H)
    xs, ys = np.arange(W, dtype=F32) + F32(0.5), np.arange(H, dtype=F32) + F32(0.5)
    cx, cy = xs[None, :] + d[0], ys[:, None] + d[1]
    assert np.isfinite(cx).all() and np.isfinite(cy).all()
    ran(f"warp {W}x{H}", left=(cx < 0).sum(), right=(cx >= W).sum(), above=(cy < 0).sum(), below=(cy >= H).sum(), inside=((cx >= 0) & (cx < W)).sum())
    got = ref.warp(pr[1], d[0], d[1])
    assert_bit_equal(got, pr[1][rn.tex_idx(cy, H), rn.tex_idx(cx, W)], "warp vs restate_np")
    # (the oracle exposes no warp of its own: its loop runs on coordinates like these in the composed iterations of the fixture tests)


@pytest.mark.parametrize("W,H", SHAPES + THIN)
def test_stage_squares_and_clamped_blur(ref, orc, W, H):
    """compareSquareIm, then convolutionRowsGPUT and convolutionColumnsGPUT (clamp-addressed texture taps), against orc.conv(..., 'clamp')."""
    pl, _, _ = inputs(W, H)
    g = orc.gauss_taps()
    sq = ref.square(pl[0])
    assert_bit_equal(sq, (pl[0] * pl[0]).astype(F32), "square")
    rows = ref.rows_t(sq)
    assert_bit_equal(rows, rn.conv1d(sq, g, -1, "clamp"), "rows T vs restate_np")
    both = ref.cols_t(rows)
    assert_bit_equal(both, orc.conv(sq, g, "clamp"), "rows T + columns T vs oracle")
    assert_bit_equal(both, rn.blur(sq, g, "clamp"), "rows T + columns T vs restate_np")


@pytest.mark.parametrize("W,H", SHAPES + THIN)
def test_stage_products_and_zero_padded_blur(ref, orc, W, H):
    """compareImMove with all five moves, then the shared-memory convolutionRowsGPU / convolutionColumnsGPU (run with real threads and a
    barrier, on a zero canvas: see tests/ref_stages.py), against orc.conv_rows_zero / conv_cols_zero."""
    pl, pr, d = inputs(W, H)
    g = orc.gauss_taps()
    warped = ref.warp(pr[2], d[0], d[1])
    for mx, my in rs.MOVES:
        prod = ref.compare_move(pl[2], warped, mx, my)
        assert_bit_equal(prod, (pl[2] * rn.shift_clamped(warped, int(mx), int(my))).astype(F32), f"product move {mx, my}")
        rows = ref.smem_rows(prod)
        assert_bit_equal(rows, orc.conv_rows_zero(prod, g), f"smem rows {mx, my} vs oracle")
        both = ref.smem_cols(rows)
        assert_bit_equal(both, orc.conv_cols_zero(rows, g), f"smem columns {mx, my} vs oracle")
        assert_bit_equal(both, rn.blur(prod, g, "zero"), f"smem blur {mx, my} vs restate_np")


def test_shared_memory_convolutions_as_the_host_calls_them(ref, orc):
    """SURVEY.md section 9, U2 / U3, asserted as the deviation it is.  Called the way MatchGPULib.cpp:912-925 / 1932-1945 calls them (pitch = W, a
    ragged 37 x 29 image) the two kernels load their main tiles without bounds checks (MatchLib.cu:97-100, 220-223): taps right of the image
    read the next row's first pixels, taps below it read past the buffer.  The project (oracle, restatement, kernels) pads with zeros instead,
    as the reference's own CPU convolution does.  Here: away from those taps the literal call equals the oracle bit for bit; at them it equals
    the oracle's sum continued with the taps the kernel really read; and the rows kernel's partial-block stores (:125-137) reach past the row
    end, so columns 0..14 of later rows are excluded from the comparison of the literal call."""
    W, H = 37, 29
    pl, _, _ = inputs(W, H)
    g = orc.gauss_taps()
    src = pl[0]
    fill = F32(1000.0)
    rows = ref.smem_literal("convolutionRowsGPU", src, fill)
    exp = orc.conv_rows_zero(src, g)
    assert_bit_equal(rows[:, 15:W - 2], exp[:, 15:W - 2], "rows, away from U2")
    assert_bit_equal(rows[0, :W - 2], exp[0, :W - 2], "rows, first row")
    nxt = np.concatenate([src[1:, :2], np.full((1, 2), fill, F32)])  # what lies behind each row's end: the next row, then the slack
    u2_a = (exp[:, W - 2] + g[0] * nxt[:, 0]).astype(F32)                                   # column W - 2: tap j = 2 reads next[0]
    u2_b = ((exp[:, W - 1] + g[1] * nxt[:, 0]).astype(F32) + g[0] * nxt[:, 1]).astype(F32)  # column W - 1: taps j = 1, 2
    assert_bit_equal(rows[:, W - 2], u2_a, "rows, U2 at column W - 2")
    assert_bit_equal(rows[:, W - 1], u2_b, "rows, U2 at column W - 1")
    assert (rows[:, W - 2:] != exp[:, W - 2:]).all()
    cols = ref.smem_literal("convolutionColumnsGPU", src, fill)
    expc = orc.conv_cols_zero(src, g)
    assert_bit_equal(cols[:H - 2], expc[:H - 2], "columns, away from U3")
    u3_a = (expc[H - 2] + g[0] * fill).astype(F32)
    u3_b = ((expc[H - 1] + g[1] * fill).astype(F32) + g[0] * fill).astype(F32)
    assert_bit_equal(cols[H - 2], u3_a, "columns, U3 at row H - 2")
    assert_bit_equal(cols[H - 1], u3_b, "columns, U3 at row H - 1")


def _np_quotient(a, b, n, mx, my):
    with np.errstate(all="ignore"):
        raw = ((n * n).astype(F32) / (a * rn.shift_clamped(b, int(mx), int(my))).astype(F32)).astype(F32)
    return raw, rn.clamp01(raw)


@pytest.mark.parametrize("W,H", SHAPES + THIN)
def test_stage_correlation_three_channel_forms(ref, orc, W, H):
    """calculateImMoveCorr alone (channel 0), followed by calculateTrueDisparity (channel 1: q + Q) and by floatrescale (channel 2: (Q + q) / 3)
    as MatchGPULib.cpp:2033-2070 chains them, on operands that make the quotient NaN (0/0), exceed 1 and fall below 0 so that both clamps act."""
    rng = np.random.Generator(np.random.PCG64(W * 100 + H))
    n3 = rng.uniform(0, 300, (3, H, W)).astype(F32)
    a3 = rng.uniform(1, 300, (3, H, W)).astype(F32)
    b3 = rng.uniform(1, 300, (3, H, W)).astype(F32)
    a3[0].ravel()[::7] *= F32(-1)       # a negative denominator: quotient below 0
    a3[1].ravel()[3::11] = 0            # x / 0 = inf -> clamped to 1
    n3[1].ravel()[3::22] = 0            # 0 / 0 = NaN, stays NaN
    n3[2].ravel()[5::9] *= F32(1e-3)    # small quotients, inside (0, 1)
    a3[2].ravel()[1::13] *= F32(1e3)
    for mx, my in rs.MOVES:
        Q, seen = None, dict(nan=0, above=0, below=0, inside=0)
        for k in range(3):
            q = ref.move_corr(a3[k], b3[k], n3[k], mx, my)
            raw, want = _np_quotient(a3[k], b3[k], n3[k], mx, my)
            assert_bit_equal(q, want, f"quotient and clamp, channel {k}, move {mx, my}")
            seen = dict(nan=seen["nan"] + np.isnan(raw).sum(), above=seen["above"] + (raw > 1).sum(), below=seen["below"] + (raw < 0).sum(),
                        inside=seen["inside"] + ((raw > 0) & (raw < 1)).sum())
            if k == 0:
                Q, Qn = q, want
            elif k == 1:
                Q, Qn = ref.true_disparity(Q, q), (want + Qn).astype(F32)
            else:
                Q, Qn = ref.floatrescale(Q, q, 3.0), ((Qn + want).astype(F32) / F32(3.0)).astype(F32)
            assert_bit_equal(Q, Qn, f"channel form {k}, move {mx, my}")
        ran(f"correlation {W}x{H} move {mx, my}", **seen)


def _parabola_operands(W, H, seed):
    """Correlation triples (c, l, r) in [0, 1] that reach every branch of PolyDisparity: c1 >= 0 (a valley or flat), c1 < 0 with the vertex
    above 1 (capped) and not, a capped vertex within 1e-10 of c, a NaN."""
    rng = np.random.Generator(np.random.PCG64(seed))
    c, l, r = (rng.random((H, W)).astype(F32) for _ in range(3))
    f = lambda a: a.ravel()  # noqa: E731
    f(c)[0::5] = np.maximum(f(l)[0::5], f(r)[0::5]) + F32(0.05)        # a peak: c1 < 0
    f(c)[1::10] = F32(0.999)                                           # peaks whose fitted vertex passes 1
    f(l)[1::10], f(r)[1::10] = F32(0.2), F32(0.99)
    f(c)[2::15] = F32(0.1)                                             # a valley: c1 > 0
    f(l)[3::20] = f(r)[3::20] = f(c)[3::20]                            # flat: c1 = 0
    f(c)[4:8] = np.nan                                                 # U7
    f(c)[8:10], f(l)[8:10], f(r)[8:10] = F32(1.5), F32(1.0), F32(1.0)  # c above 1 (not produced by the clamp, but the code has the branch)
    return c, l, r


@pytest.mark.parametrize("W,H", SHAPES + THIN)
@pytest.mark.parametrize("thr", [1.0, 0.55, 0.1])
def test_stage_parabola(ref, orc, W, H, thr):
    """calculatePolyDisparity (the x and the y call differ only in their operands) against orc.poly per pixel and restate_np.poly: the
    double promotions of MatchLib.cu:813-830, the min / max clamp in double, the three branches."""
    c, l, r = _parabola_operands(W, H, W + H + int(thr * 100))
    thr = float(F32(thr))
    delta, corr = ref.poly(l, r, c, thr)
    nd, nc = rn.poly(c, l, r, F32(thr))
    assert_bit_equal(delta, nd, "delta vs restate_np")
    assert_bit_equal(corr, nc, "corr vs restate_np")
    od, oc = np.empty_like(delta), np.empty_like(corr)
    for i in range(c.size):
        od.ravel()[i], oc.ravel()[i] = orc.poly(c.ravel()[i], l.ravel()[i], r.ravel()[i], thr)
    assert_bit_equal(delta, od, "delta vs oracle")
    assert_bit_equal(corr, oc, "corr vs oracle")
    with np.errstate(all="ignore"):
        b1 = ((r - l) / F32(2)).astype(F32)
        c1 = (r - (c + b1)).astype(F32)
    ran(f"parabola {W}x{H} thr {thr:.2f}", valley_or_flat=(c1 >= 0).sum(), capped=((c1 < 0) & (corr == 1)).sum(),
        peak_below_one=((c1 < 0) & (corr < 1)).sum(), nan=np.isnan(c1).sum(), clamped_to_threshold=((c1 < 0) & (np.abs(delta) == F32(thr))).sum())


@pytest.mark.parametrize("W,H", SHAPES + THIN)
def test_stage_product_update_and_confidence_blend(ref, orc, W, H):
    """compCorrelation, scaleDisparity (m = 1), calculateTrueDisparity and calculateTrueConfidence: the blend 0.75 * old + 0.25 * new in
    double, on confidences that land above 1 and below 0 so that both clamps act."""
    _, _, d = inputs(W, H)
    rng = np.random.Generator(np.random.PCG64(W + 31 * H))
    cx, cy = (0.4 + 0.6 * rng.random((H, W))).astype(F32), (0.4 + 0.6 * rng.random((H, W))).astype(F32)
    dd = rng.normal(0, 0.5, (H, W)).astype(F32)
    old = d[2].copy()
    old.ravel()[::6], old.ravel()[1::6] = F32(1.5), F32(-0.5)
    kap = ref.comp_correlation(cx, cy)
    assert_bit_equal(kap, (cy * cx).astype(F32), "compCorrelation")
    assert_bit_equal(ref.scale_disparity(dd, 1), dd, "scaleDisparity, m = 1")
    assert_bit_equal(ref.true_disparity(dd, d[0]), (d[0] + dd).astype(F32), "calculateTrueDisparity")
    v = (0.75 * old.astype(np.float64) + 0.25 * kap.astype(np.float64)).astype(F32)
    ran(f"blend {W}x{H}", above_one=(v > 1).sum(), below_zero=(v < 0).sum(), inside=((v > 0) & (v < 1)).sum())
    assert_bit_equal(ref.true_confidence(kap, old), rn.clamp01(v), "calculateTrueConfidence")
    in_float = rn.clamp01((F32(0.75) * old + F32(0.25) * kap).astype(F32))
    assert (in_float != rn.clamp01(v)).any(), "these operands cannot tell a float blend from the double one"


@pytest.mark.parametrize("W,H", SHAPES + THIN)
def test_stage_smooth_and_box(ref, orc, W, H):
    """smooth on all three planes for five passes (zero, negative and 1e-30 confidences: 0/0 spreads as NaN through the VALUES, never through
    a coordinate), then the box by convolutionRowsGPUTa / convolutionColumnsGPUTa, against orc.smooth_pass / orc.box3 and restate_np."""
    cur = rs.conf_field(W, H, 7300 + W)
    five = [cur[2], *(rn.shift_clamped(cur[2], sx, sy) for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1)))]
    zero_sum = (sum(np.abs(a) for a in five) == 0)[1:, 1:]
    if min(W, H) > 1:
        ran(f"smooth {W}x{H}", zero_weight_sum=zero_sum.sum(), negative=(cur[2] < 0).sum(), tiny=(cur[2] == F32(1e-30)).sum(), frame=W + H - 1)
    else:  # a one-pixel-wide image is all frame (ix > 0 && iy > 0 never holds): the kernel stores nothing
        assert_bit_equal(ref.smooth3(cur), cur, "thin image: nothing smoothed")
    with np.errstate(all="ignore"):
        for p in range(1, 6):
            nxt = ref.smooth3(cur)
            assert_bit_equal(nxt, orc.smooth_pass(cur), f"pass {p} vs oracle")
            assert_bit_equal(nxt, rn.smooth_pass(cur), f"pass {p} vs restate_np")
            cur = nxt
            box = ref.box3(cur)
            assert_bit_equal(box, orc.box3(cur), f"box after pass {p} vs oracle")
            assert_bit_equal(box, np.stack([rn.blur(a, rn.BOX, "clamp") for a in cur]), f"box after pass {p} vs restate_np")
    if min(W, H) > 1:
        assert np.isnan(cur).any()


def test_stage_pyramid(ref, orc):
    """Levels 1 to 3 by convolutionRowsGPU, convolutionColumnsGPU and subsampleGPU against orc.pyramid and restate_np.pyramid.  subsampleGPU
    stores nothing where the source coordinate is not inside the image (MatchLib.cu:330-338); for the reference's level sizes that never
    happens -- asserted: no pixel keeps the NaN the destination was filled with."""
    for W, H in SHAPES:
        pl, _, _ = inputs(W, H)
        got = ref.pyramid(pl, 4, orc.level_dims(W, H, 4))
        exp, exn = orc.pyramid(pl, 4), rn.pyramid(pl, 4)
        for lev in (1, 2, 3):
            assert not np.isnan(got[lev]).any()
            assert_bit_equal(got[lev], exp[lev], f"{W}x{H} level {lev} vs oracle")
            assert_bit_equal(got[lev], exn[lev], f"{W}x{H} level {lev} vs restate_np")


def test_stage_seed_and_upsample(ref, orc):
    """subsampleDispGPU against orc.seed and restate_np.seed; the same call cropped as foveatedsubsampleDisp crops it (MatchGPULib.cpp:1612-1644)
    against orc.seed_fovea; partsubsampleDispGPU against the upsampling inside orc.reconstruct_full (hierarchicalDisparity, :2638-2667).

    partsubsampleDispGPU is NOT what seeds a fovea level in the reference: it divides the coordinate by (float)SCALE and multiplies in float,
    subsampleDispGPU multiplies the coordinate by (float)(1 / SCALE) and the value by the double SCALE.  The two are compared below and differ,
    so orc.seed_fovea is pinned to the call the host makes."""
    sf = F32(1 / rs.SCALE)
    for W, H in SHAPES:
        _, _, d = inputs(W, H)
        for W2, H2 in ((int(W * rs.SCALE) + 1, int(H * rs.SCALE) + 1), (int(W * rs.SCALE), int(H * rs.SCALE))):
            got = np.stack([ref.subsample_disp(p, W2, H2, sf) for p in d])
            assert_bit_equal(got, orc.seed(d, W2, H2), f"seed {W}x{H} -> {W2}x{H2} vs oracle")
            assert_bit_equal(got, rn.seed(d, W2, H2), f"seed {W}x{H} -> {W2}x{H2} vs restate_np")
        Wup, Hup = int(W * rs.SCALE) + 1, int(H * rs.SCALE) + 1
        up = np.stack([ref.subsample_disp(p, Wup, Hup, sf) for p in d])
        for l, u in ((Wup // 2 - W // 2, Hup // 2 - H // 2), (0, 0), (Wup - W, Hup - H)):
            assert_bit_equal(up[:, u:u + H, l:l + W], orc.seed_fovea(d, Wup, Hup, l, u), f"fovea seed {W}x{H} at {l, u}")
        # hierarchicalDisparity with two levels: level 1 (the whole frame at W x H) upsampled to level 0, the fovea pasted over its window
        assert orc.level_dims(Wup, Hup, 2) == ([Wup, W], [Hup, H])
        stack = np.stack([np.stack([np.zeros_like(p), p]) for p in d])  # (3, F = 2, H, W): level 0 (the fovea) zeros, level 1 the field
        full = orc.reconstruct_full(stack, Wup, Hup, 2)
        part = np.stack([ref.partsubsample_disp(p, Wup, Hup, F32(rs.SCALE)) for p in d])
        _, _, ox, oy, _, _ = orc.fovea_geometry(Wup, Hup, 2, 2)
        window = np.zeros((Hup, Wup), bool)
        window[oy[0]:oy[0] + H, ox[0]:ox[0] + W] = True
        assert_bit_equal(full[:, ~window], part[:, ~window], f"upsampling of reconstruct_full {W}x{H}")
        assert (full[:, window] == 0).all()
        differ = int((part.view(np.uint32) != up.view(np.uint32)).sum())
        print(f"partsubsampleDispGPU vs subsampleDispGPU {W}x{H} -> {Wup}x{Hup}: {differ} of {part.size} values differ")
        assert differ > 0


# ---- one composed iteration, and the fixture -------------------------------------------------------------------------------------------------

_live = {}


def live_outputs(ref, orc, gold):
    """The fixture's outputs computed now by the reference's stage code (once per session: about ten seconds)."""
    if "out" not in _live:
        inp = {k: gold[k] for k in gold.files if k.endswith(("_L", "_R", "_d0")) or k == "smooth_src"}
        t = time.perf_counter()
        _live["out"] = rs.live_fixture_outputs(ref, inp, orc.threshold_schedule(rs.MI), orc.level_dims)
        print(f"reference stages, all fixture cases: {time.perf_counter() - t:.1f} s")
    return _live["out"]


def oracle_outputs(orc, gold):
    def it(pl, pr, d0, top):
        d, dbg = orc.iterate_level(pl, pr, d0, rs.MI, rs.S_PASSES, top, 1, 2, want_dbg=True)
        return d, dbg[:5], dbg[5:]
    return rs.fixture_outputs(gold, it, lambda p0: orc.pyramid(p0, 4), orc.seed, orc.smooth_pass, orc.box3)


def restate_outputs(gold):
    def it(pl, pr, d0, top):
        return rn.iterate_level(pl, pr, d0, 0, bool(top), 1, 2, mi=rs.MI, S=rs.S_PASSES, want_dbg=True)
    return rs.fixture_outputs(gold, it, lambda p0: rn.pyramid(p0, 4), rn.seed, rn.smooth_pass,
                              lambda d: np.stack([rn.blur(p, rn.BOX, "clamp") for p in d]))


def _same_as_fixture(out, gold, who):
    keys = [k for k in gold.files if not (k.endswith(("_L", "_R", "_d0")) or k == "smooth_src")]
    assert sorted(keys) == sorted(out), f"{who}: the fixture holds {sorted(set(keys) ^ set(out))} more or less than the cases of tests/ref_stages.py"
    for k in keys:
        assert_bit_equal(out[k], gold[k], f"{who}: {k}")


def test_fixture_inputs_are_the_documented_ones(gold):
    """The stored inputs are the ones tests/ref_stages.py builds (uint8 images, float seed fields), and the file stays small."""
    for k, v in rs.fixture_inputs().items():
        assert gold[k].dtype == v.dtype and (gold[k].view(np.uint8) == v.view(np.uint8)).all(), k
    assert os.path.getsize(os.path.join(GOLDEN, "ref_stages.npz")) < 1 << 20


def test_fixture_branches(gold, orc):
    """The composed cases reach every branch: warps past all four borders, 0/0 quotients, all three parabola branches, blends above 1 and below
    0; and the field that re-enters as texture coordinates stays finite (no NaN coordinate is ever given to the reference library)."""
    thr = orc.threshold_schedule(rs.MI)
    capped = 0
    for W, H in rs.ITERATE_CASES:
        c = f"{W}x{H}"
        pl, pr, d = rs.planes(gold[c + "_L"]), rs.planes(gold[c + "_R"]), gold[c + "_d0"]
        for top in (0, 1):
            for m in (1, 2):
                assert np.isfinite(d).all()
                cx, cy = np.arange(W, dtype=F32) + F32(0.5) + d[0], (np.arange(H, dtype=F32) + F32(0.5))[:, None] + d[1]
                nxt, dbg = orc.iterate_level(pl, pr, d, rs.MI, rs.S_PASSES, top, m, m, want_dbg=True)
                Q = dbg[:5]
                with np.errstate(all="ignore"):
                    corr = np.stack([rn.poly(Q[4], Q[0], Q[1], thr[m - 1])[1], rn.poly(Q[4], Q[2], Q[3], thr[m - 1])[1]])
                    v = 0.75 * d[2].astype(np.float64) + 0.25 * (corr[0] * corr[1]).astype(np.float64)
                seen = dict(left=(cx < 0).sum(), right=(cx >= W).sum(), above=(cy < 0).sum(), below=(cy >= H).sum(), nan_quotient=np.isnan(Q).sum(),
                            valley=(corr == F32(0.4)).sum(), peak=((corr != F32(0.4)) & (corr < 1)).sum())
                capped += int((corr == 1).sum())
                if m == 1 and not top:  # the seed field's own patches; later iterations carry what the smoothing left of them
                    seen.update(blend_above_one=(v > 1).sum(), blend_below_zero=(v < 0).sum())
                ran(f"composed {c} top={top} m={m}", **seen)
                d = nxt
            d = gold[c + "_d0"]
        assert np.isfinite(gold[c + "_top0"]).all() and np.isfinite(gold[c + "_top1"]).all()
    ran("composed, all cases (a fitted vertex above 1 is rare on real quotients)", capped=capped)


def test_fixture_vs_oracle(gold, orc):
    """The C oracle gives the bits that the reference's stage code gave: two composed iterations (mi = 4, S = 5, with and without is_top) at Q,
    at (dx', dy', kappa) and at the final field; pyramid levels 1 to 3; seeds; one to five smoothing passes with and without the box."""
    _same_as_fixture(oracle_outputs(orc, gold), gold, "oracle")


def test_fixture_vs_restate_np(gold):
    _same_as_fixture(restate_outputs(gold), gold, "restate_np")


def test_oracle_and_restate_np_vs_live_reference(ref, orc, gold):
    """The composed iterations (Q, (dx', dy', kappa) and the final field), the pyramid, the seeds and the smoothing passes of the oracle and of
    restate_np against what the reference's stage code computes NOW, without the stored outputs in between."""
    live = live_outputs(ref, orc, gold)
    for who, out in (("oracle", oracle_outputs(orc, gold)), ("restate_np", restate_outputs(gold))):
        assert sorted(out) == sorted(live)
        for k in live:
            assert_bit_equal(out[k], live[k], f"{who} vs live reference: {k}")


def test_fixture_vs_live_reference(ref, orc, gold):
    """Where the library was built: it still gives what the fixture holds (the composition driver of tests/ref_stages.py, the stand-in headers
    and the compiler flags have not moved)."""
    _same_as_fixture(live_outputs(ref, orc, gold), gold, "live reference")
