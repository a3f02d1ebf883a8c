"""Calls the reference's own stage functions (MatchLib.cu compiled for the CPU: oracle/_ref/libmatchlib_cpu.so, oracle/ref_cpu/) on numpy
arrays -- test infrastructure, shared by tests/test_ref_pin_host.py and tests/golden/make_golden.py.

Every method is one extern "C" function of MatchLib.cu with the argument roles that MatchGPULib.cpp gives it (file:line cited per method).
iterate() and pyramid() compose those calls in the order of the reference's host code.  The composition is THIS file's code: the order of
the calls, the buffers that alias, the taps (MatchGPULib.cpp:761-774, 344-348) and the threshold schedule (:2299-2306) are restated here
from the cited lines, so what THIS file pins is the arithmetic of every stage.  The host's own ordering is pinned elsewhere: the host class
itself runs on the CPU as oracle/_ref/ref_driver (oracle/ref_cpu/ref_driver.cpp, tests/ref_driver.py), whole calls of it are frozen in
tests/golden/ref_driver_*.npz, and the oracle -- whose steps this file's composition equals bit for bit -- is held to those.

The two shared-memory convolutions are only defined by the reference where the width is a multiple of 128 and the height a multiple of 64
(elsewhere their unguarded loads read the next row or past the buffer and their stores race).  smem_rows / smem_cols
therefore run them on a zero canvas of such a size with the image in its top left corner -- the zero padding that U2 / U3 resolve to, made
explicit in the input -- and return the image's part; smem_literal runs them as they are, on buffers with slack, to show the deviation itself.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

F32 = np.float32
MOVES = [(-1.0, 0.0), (1.0, 0.0), (0.0, -1.0), (0.0, 1.0), (0.0, 0.0)]  # MatchGPULib.cpp:1677 with threshold = 1.0 (:1673)
SCALE = 1.41421356  # MatchLib_common.h:15

_V, _I, _F = C.c_void_p, C.c_int, C.c_float
_SIGNATURES = {  # MatchLib.cu's extern "C" prototypes
    "setConvolutionKernel": [_V], "setConvolutionAverageKernel": [_V],
    "convolutionRowsGPU": [_V, _V, _I, _I], "convolutionColumnsGPU": [_V, _V, _I, _I],
    "subsampleGPU": [_V, _V, _I, _I, _F, _I, _I], "subsampleDispGPU": [_V, _V, _I, _I, _F, _I, _I],
    "partsubsampleDispGPU": [_V, _V, _I, _I, _F, _I, _I],
    "warp": [_V, _V, _V, _V, _I, _I], "compareSquareIm": [_V, _V, _I, _I],
    "compareImMove": [_V, _V, _V, _I, _I, _F, _F], "calculateImMoveCorr": [_V, _V, _V, _V, _I, _I, _F, _F],
    "calculatePolyDisparity": [_V, _V, _V, _V, _V, _I, _I, _F], "compCorrelation": [_V, _V, _V, _I, _I],
    "calculateTrueDisparity": [_V, _V, _V, _I, _I], "calculateTrueConfidence": [_V, _V, _V, _I, _I],
    "scaleDisparity": [_V, _V, _I, _I, _I], "smooth": [_V, _V, _V, _I, _I], "floatrescale": [_V, _V, _V, _F, _I, _I],
    "convolutionRowsGPUT": [_V, _V, _I, _I], "convolutionColumnsGPUT": [_V, _V, _I, _I],
    "convolutionRowsGPUTa": [_V, _V, _I, _I], "convolutionColumnsGPUTa": [_V, _V, _I, _I],
}


def _up(n, m):
    return -(-n // m) * m


class RefStages:
    def __init__(self, lib, gauss, box):
        self.lib = lib
        for name, args in _SIGNATURES.items():
            f = getattr(lib, name)
            f.argtypes, f.restype = args, None
        lib.cpu_array_wrap.argtypes, lib.cpu_array_wrap.restype = [_V, _I, _I], _V
        lib.cpu_array_free.argtypes, lib.cpu_array_free.restype = [_V], None
        self._taps = (np.ascontiguousarray(gauss, F32), np.ascontiguousarray(box, F32))
        lib.setConvolutionKernel(self._taps[0].ctypes.data)         # MatchGPULib.cpp:775
        lib.setConvolutionAverageKernel(self._taps[1].ctypes.data)  # :349

    # ---- plumbing: out = stage(textures..., scalars...) -------------------------------------------------------------------------------------
    def _run(self, name, outs, texs, *scalars, pre=()):
        """Calls `name`(outs..., cudaArrays of texs..., pre..., W, H, scalars...) and returns the outputs."""
        H, W = np.shape(texs[0])
        keep = [np.ascontiguousarray(t, F32) for t in texs]
        hs = [self.lib.cpu_array_wrap(t.ctypes.data, t.shape[1], t.shape[0]) for t in keep]
        try:
            getattr(self.lib, name)(*[o.ctypes.data for o in outs], *hs, *pre, W, H, *scalars)
        finally:
            for h in hs:
                self.lib.cpu_array_free(h)
        return outs[0] if len(outs) == 1 else tuple(outs)

    @staticmethod
    def _new(like, fill=np.nan):
        return np.full(np.shape(like), fill, F32)  # NaN where a stage stores nothing

    # ---- the stages ----------------------------------------------------------------------------------------------------------------------------
    def warp(self, right, dx, dy):  # MatchGPULib.cpp:1792-1799
        return self._run("warp", [self._new(right)], [right, dx, dy])

    def square(self, img):  # :1809-1821
        return self._run("compareSquareIm", [self._new(img)], [img])

    def rows_t(self, img):  # :1866, :1887
        return self._run("convolutionRowsGPUT", [self._new(img)], [img])

    def cols_t(self, img):  # :1875, :1896
        return self._run("convolutionColumnsGPUT", [self._new(img)], [img])

    def rows_ta(self, img):  # :2362 ...
        return self._run("convolutionRowsGPUTa", [self._new(img)], [img])

    def cols_ta(self, img):  # :2371 ...
        return self._run("convolutionColumnsGPUTa", [self._new(img)], [img])

    def compare_move(self, left, warped, mx, my):  # :1917-1925
        return self._run("compareImMove", [self._new(left)], [left, warped], mx, my)

    def move_corr(self, a, b, n, mx, my):  # :2019-2043: dispx = A, dispy = B, a_Src = blurred product
        return self._run("calculateImMoveCorr", [self._new(a)], [a, b, n], mx, my)

    def true_disparity(self, warpy, src):  # :2051-2057, :2206-2220: src + warpy
        return self._run("calculateTrueDisparity", [self._new(src)], [warpy, src])

    def floatrescale(self, src, rst, m):  # :2062-2069: (src + rst) / m
        return self._run("floatrescale", [self._new(src)], [src, rst], pre=(m,))

    def poly(self, lo, hi, centre, thr):  # :2129-2152: dispx = l, dispx2 = r, d_Src = c -> (delta, corr)
        return self._run("calculatePolyDisparity", [self._new(lo), self._new(lo)], [lo, hi, centre], thr)

    def comp_correlation(self, warpy, src):  # :2159-2165
        return self._run("compCorrelation", [self._new(src)], [warpy, src])

    def scale_disparity(self, src, m):  # :2175-2189, m = (int)thresholdtest = 1
        return self._run("scaleDisparity", [self._new(src)], [src], pre=(int(m),))

    def true_confidence(self, warpy, src):  # :2243-2249: 0.75 * src + 0.25 * warpy, src = the old confidence
        return self._run("calculateTrueConfidence", [self._new(src)], [warpy, src])

    def smooth(self, src, conf):  # :2269-2289: the destination is the buffer the texture was copied from (:2264-2266)
        return self._run("smooth", [np.ascontiguousarray(src, F32).copy()], [src, conf])

    def _resample(self, name, src, W2, H2, sf):
        out = np.full((H2, W2), np.nan, F32)
        s = np.ascontiguousarray(src, F32)
        h = self.lib.cpu_array_wrap(s.ctypes.data, s.shape[1], s.shape[0])
        try:
            getattr(self.lib, name)(out.ctypes.data, h, s.shape[1], s.shape[0], float(F32(sf)), W2, H2)
        finally:
            self.lib.cpu_array_free(h)
        return out

    def subsample(self, src, W2, H2, sf):  # :1003-1011
        return self._resample("subsampleGPU", src, W2, H2, sf)

    def subsample_disp(self, src, W2, H2, sf):  # :1562-1570, :1628-1636
        return self._resample("subsampleDispGPU", src, W2, H2, sf)

    def partsubsample_disp(self, src, W2, H2, sf):  # :2666-2667
        return self._resample("partsubsampleDispGPU", src, W2, H2, sf)

    # ---- the shared-memory convolutions ----------------------------------------------------------------------------------------------------
    def _smem(self, name, img):
        H, W = img.shape
        can = np.zeros((_up(H, 64), _up(W, 128)), F32)
        can[:H, :W] = img
        out = np.full(can.shape, np.nan, F32)
        getattr(self.lib, name)(out.ctypes.data, can.ctypes.data, can.shape[1], can.shape[0])
        assert np.isnan(can).any() or not np.isnan(out).any(), "a canvas pixel was not stored"
        return np.ascontiguousarray(out[:H, :W])

    def smem_rows(self, img):  # :912-917, :1932-1937
        return self._smem("convolutionRowsGPU", img)

    def smem_cols(self, img):  # :920-925, :1940-1945
        return self._smem("convolutionColumnsGPU", img)

    def smem_literal(self, name, img, fill):
        """convolutionRowsGPU / convolutionColumnsGPU exactly as the host calls them (pitch = W, buffers of W * H floats), on buffers that
        continue with `fill` far enough for every unguarded load and store of U2 / U3 to land in memory this call owns."""
        H, W = img.shape
        n = (_up(H, 64) + 80) * max(W, 16) + _up(W, 128) + 512
        src, dst = np.full(n, fill, F32), np.full(n, np.nan, F32)
        src[:H * W] = np.ascontiguousarray(img, F32).ravel()
        getattr(self.lib, name)(dst.ctypes.data, src.ctypes.data, W, H)
        return dst[:H * W].reshape(H, W).copy()

    def blur_smem(self, img):
        return self.smem_cols(self.smem_rows(img))

    # ---- compositions (this file's own ordering, after MatchGPULib.cpp) -----------------------------------------------------------------------
    def pyramid(self, planes0, levels, dims):
        """CreatePyramidFromImage, MatchGPULib.cpp:1063-1106: level 1 from blur(level 0) at (float)SCALE, level i + 2 from blur(level i) at 2.0f."""
        w, h = dims
        out = [np.ascontiguousarray(planes0, F32)] + [None] * (levels - 1)
        for i in range(levels):
            need1, need2 = (i == 0 and levels > 1), (i + 2 < levels)
            if not (need1 or need2):
                continue
            blurred = [self.blur_smem(p) for p in out[i]]
            if need1:
                out[1] = np.stack([self.subsample(b, w[1], h[1], F32(SCALE)) for b in blurred])
            if need2:
                out[i + 2] = np.stack([self.subsample(b, w[i + 2], h[i + 2], F32(0.000 + int(SCALE * SCALE + 0.5))) for b in blurred])
        return out

    def cost(self, L3, R3, dx, dy):
        """MatchGPULib.cpp:1745-2084 (usingMoreGPUMemory == 1): the five correlation planes of one iteration."""
        Q = [None] * 5
        for j in range(3):
            warped = self.warp(R3[j], dx, dy)                                   # :1792; compare := c (:1802)
            a = self.cols_t(self.rows_t(self.square(L3[j])))                    # :1809, :1866-1880 -> texturel (:1904)
            b = self.cols_t(self.rows_t(self.square(warped)))                   # :1816, :1887-1901 -> texturer (:1905)
            for i, (mx, my) in enumerate(MOVES):
                n = self.blur_smem(self.compare_move(L3[j], warped, mx, my))    # :1917-1945 -> texturelr (:1972)
                q = self.move_corr(a, b, n, mx, my)                             # :2019 (j != 0) / :2034 (j == 0)
                if j == 0:
                    Q[i] = q
                elif j == 1:
                    Q[i] = self.true_disparity(Q[i], q)                         # :2049-2057: texturelr = temp, temp2 = l
                else:
                    Q[i] = self.floatrescale(Q[i], q, 3.0)                      # :2060-2069
        return Q

    def update(self, Q, d3, thr, blend):
        """MatchGPULib.cpp:2129-2250: parabolas, correlation product, update, confidence blend -> (dx', dy', kappa)."""
        ddx, cx = self.poly(Q[0], Q[1], Q[4], thr)                              # :2129: texturel, texturer, texturelr
        ddy, cy = self.poly(Q[2], Q[3], Q[4], thr)                              # :2143: a_Src, compare, texturelr
        kap = self.comp_correlation(cx, cy)                                     # :2156-2165: dispy = texturel = r, a_Src = texturer = c
        ddx, ddy = self.scale_disparity(ddx, 1), self.scale_disparity(ddy, 1)   # :2175-2189, thresholdtest = step = 1.0 (:1261)
        ndx = self.true_disparity(ddx, d3[0])                                   # :2206: dispy = texturel = l, a_Src = disp0
        ndy = self.true_disparity(ddy, d3[1])                                   # :2214
        if blend:                                                               # :2223: not ((level == 0) && (m == 1))
            kap = self.true_confidence(kap, d3[2])                              # :2229-2249: dispy = texturelr = c, a_Src = disp2
        return np.stack([ndx, ndy, kap])

    def smooth3(self, d3):  # :2264-2289: all three planes from the pre-pass snapshot
        return np.stack([self.smooth(d3[0], d3[2]), self.smooth(d3[1], d3[2]), self.smooth(d3[2], d3[2])])

    def box3(self, d3):  # :2361-2412
        return np.stack([self.cols_ta(self.rows_ta(p)) for p in d3])

    def iterate(self, L3, R3, d3, thresholds, S, is_top, m_from, m_to):
        """Iterations m_from..m_to of matchlevel -> (field, Q of the last iteration, (dx', dy', kappa) of the last iteration)."""
        d = np.ascontiguousarray(d3, F32).copy()
        Q = nd = None
        for m in range(m_from, m_to + 1):
            Q = self.cost(L3, R3, d[0], d[1])
            nd = self.update(Q, d, float(thresholds[m - 1]), not (is_top and m == 1))
            cur = nd
            for _ in range(S):
                cur = self.smooth3(cur)
            d = self.box3(cur)
        return d, np.stack(Q), nd


def load(orc):
    """RefStages over the live library with the project's taps, or None where the library was not built."""
    lib = orc.matchlib_cpu()
    return None if lib is None else RefStages(lib, orc.gauss_taps(), orc.box_taps())


# ---- inputs that make every branch run (tests/test_ref_pin_host.py asserts that each did) ----------------------------------------------------

def pair(W, H, seed):
    """A textured [1, 255] pair with a zero patch in each image: 0/0 in the correlation quotient -> NaN -> the parabola's 0.4 branch (U7)."""
    from ug_stereomatcher_amd import synth
    L, R, _, _ = synth.make_pair(max(W, 16), max(H, 16), seed)
    L, R = np.ascontiguousarray(L[:H, :W]), np.ascontiguousarray(R[:H, :W])
    L[H // 5:H // 5 + 7, W // 6:W // 6 + 8] = 0
    R[H // 2:H // 2 + 7, W // 2:W // 2 + 9] = 0
    return L, R


def seed_field(W, H, seed):
    """(dx, dy, conf) for the composed iterations: finite disparities that reach past all four borders; confidence with a zero patch, a 1e-30
    patch, a patch above 1 (the blend then lands above 1) and negative 2 x 2 blocks (the blend lands below 0 and is clamped to 0; a block that
    small leaves every pixel a neighbour of positive weight, so no 0/0 enters the field and no NaN becomes a texture coordinate)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = np.stack([rng.normal(0, 4, (H, W)), rng.normal(0, 3, (H, W)), 0.1 + 0.9 * rng.random((H, W))]).astype(F32)
    d[0, :, :2] -= 6
    d[0, :, -2:] += 6
    d[1, :2, :] -= 5
    d[1, -2:, :] += 5
    d[2, H // 3:H // 3 + 4, W // 4:W // 4 + 10] = 0.0
    d[2, (2 * H) // 3:(2 * H) // 3 + 3, W // 8:W // 8 + 12] = 1e-30
    d[2, H // 8:H // 8 + 3, W // 2:W // 2 + 9] = 1.5
    for k in range(4):
        y, x = (H * (2 * k + 1)) // 9, (W * (2 * k + 3)) // 11
        d[2, y:y + 2, x:x + 2] = -0.25
    return d


def conf_field(W, H, seed):
    """The field of tests/test_gpu_smooth_io.py (confidences of zero at the frame and inside, negative and 1e-30 patches) without its NaNs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = np.stack([rng.normal(0, 3, (H, W)), rng.normal(0, 3, (H, W)), 0.1 + 0.9 * rng.random((H, W))]).astype(F32)
    d[2, H // 3:H // 3 + 9, W // 4:W // 4 + 40] = 0.0
    d[2, 0:5, 0:7] = 0.0
    d[2, max(H - 6, 0):, max(W - 9, 0):] = 0.0
    d[2, H // 2:H // 2 + 3, W // 2:W // 2 + 30] = -0.25
    d[2, (2 * H) // 3:(2 * H) // 3 + 3, W // 8:W // 8 + 30] = 1e-30
    return d


# ---- the fixture tests/golden/ref_stages.npz: what the reference's code gives for stored inputs ------------------------------------------------

ITERATE_CASES = [(37, 29), (61, 45), (130, 75)]  # Q and (dx', dy', kappa) are stored for the first only
MI, S_PASSES = 4, 5
SEED_SRC, SEED_DST, SEED_DST_ODD, SEED_CROP = (37, 29), (53, 42), (52, 41), (8, 7)  # int(53 / SCALE), int(42 / SCALE) = 37, 29


def fixture_inputs():
    out = {}
    for k, (W, H) in enumerate(ITERATE_CASES):
        out[f"{W}x{H}_L"], out[f"{W}x{H}_R"] = pair(W, H, 9100 + k)
        out[f"{W}x{H}_d0"] = seed_field(W, H, 9200 + k)
    out["smooth_src"] = conf_field(37, 29, 9300)
    return out


def fixture_outputs(inp, iterate, pyramid, seed, smooth_pass, box3):
    """The fixture's outputs by any implementation: iterate(L3, R3, d0, is_top) -> (field, Q, nd) for two iterations of mi = 4, S = 5;
    pyramid(planes0) -> levels 0..3; seed(src3, W2, H2) -> field; smooth_pass(d3), box3(d3)."""
    out = {}
    for W, H in ITERATE_CASES:
        c = f"{W}x{H}"
        pl, pr = planes(inp[c + "_L"]), planes(inp[c + "_R"])
        for top in (0, 1):
            d, Q, nd = iterate(pl, pr, inp[c + "_d0"], top)
            out[f"{c}_top{top}"] = d
            if (W, H) == ITERATE_CASES[0] and Q is not None:
                out[f"{c}_Q_top{top}"], out[f"{c}_nd_top{top}"] = Q, nd
    pyr = pyramid(planes(inp["130x75_L"]))
    for lev in (1, 2, 3):
        out[f"pyr{lev}"] = pyr[lev]
    src = inp["37x29_d0"]
    out["seed_53x42"] = seed(src, *SEED_DST)
    out["seed_52x41"] = seed(src, *SEED_DST_ODD)
    with np.errstate(all="ignore"):
        cur = inp["smooth_src"]
        for p in range(1, 6):
            cur = smooth_pass(cur)
            out[f"smooth_p{p}_b0"], out[f"smooth_p{p}_b1"] = cur, box3(cur)
    return out


def planes(rgb):
    """MatchGPULib.cpp:332-338: (H, W, 3) uint8 -> three float planes"""
    return np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(F32)


def live_fixture_outputs(ref, inp, thresholds, dims):
    """fixture_outputs by the reference's own stage code."""
    def seed(src3, W2, H2):
        return np.stack([ref.subsample_disp(p, W2, H2, F32(1 / SCALE)) for p in src3])  # scalefactor = 1 / SCALE (:1222), 3 planes (:1549)
    return fixture_outputs(inp, lambda pl, pr, d0, top: ref.iterate(pl, pr, d0, thresholds, S_PASSES, top, 1, 2),
                           lambda p0: ref.pyramid(p0, 4, dims(p0.shape[2], p0.shape[1], 4)), seed, ref.smooth3, ref.box3)
