"""CPU restatement of lens distortion in triangulation, clouds and depth (include/ugsm.h, "lens distortion") for the tests.

  - undistort: the definition, in numpy float64 with every operation rounded on its own, the result rounded to float32 once;
  - distort: the forward plumb_bob model in float64 (the tests' ground truth; no library code implements it);
  - tri_point: get3DPoint's closed form for explicit (x1, y1, x2, y2), with the source's float / double mix term by term.  numpy's
    promotion of ARRAYS is C's (float32 with float32 stays float32, anything with float64 is float64), so the expressions below are the
    source's text with arrays for a .. j, x, y, sq_d() for pow(v, 2.0) and a float64 array for the literal 2.0.  tests/test_lens_host.py
    pins it to oracle.triangulate / triangulate_fovea bit for bit;
  - triangulate / triangulate_fovea: the planes of ugsm_triangulate[_fovea] from disparities, under a lens or (lens=None) without;
  - the resized map's Z comes from tests/resize_np.resize_cubic of that Z plane, records from tests/cloud_np.records, depth from
    tests/depth_np.depth_of_z.

A lens is (K1, D1, K2, D2, iterations): K 3 x 3, D = (k1, k2, p1, p2, k3).
"""
import json
import os

import numpy as np

F32, F64 = np.float32, np.float64
CAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lens_cal.json")


def rigs():
    """tests/golden/lens_cal.json: {"rig16mp": ..., "small": ...}, each with width, height, K1, D1, P1, K2, D2, P2 as arrays."""
    raw = json.load(open(CAL))
    out = {}
    for name, r in raw.items():
        if not isinstance(r, dict):
            continue
        out[name] = {k: (np.array(v, F64) if isinstance(v, list) else v) for k, v in r.items()}
        for k in ("K1", "K2"):
            out[name][k] = out[name][k].reshape(3, 3)
        for k in ("P1", "P2"):
            out[name][k] = out[name][k].reshape(3, 4)
    return out


def lens_of(rig, iterations=5):
    return rig["K1"], rig["D1"], rig["K2"], rig["D2"], iterations


def _cam(K, D):
    K = np.asarray(K, F64).reshape(9)
    k1, k2, p1, p2, k3 = (F64(v) for v in np.asarray(D, F64).reshape(5))
    return F64(K[0]), F64(K[4]), F64(K[2]), F64(K[5]), k1, k2, p1, p2, k3


def undistort64(K, D, u, v, iterations=5):
    """The iteration on float64 arrays u, v (already promoted); returns the float64 pixel coordinates before the final rounding."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = _cam(K, D)
    two, one = F64(2.0), F64(1.0)
    with np.errstate(all="ignore"):
        x0 = (u - cx) / fx
        y0 = (v - cy) / fy
        x, y = x0, y0
        for _ in range(iterations):
            r2 = x * x + y * y
            ic = one / (one + ((k3 * r2 + k2) * r2 + k1) * r2)
            dX = two * p1 * x * y + p2 * (r2 + two * x * x)
            dY = p1 * (r2 + two * y * y) + two * p2 * x * y
            x = (x0 - dX) * ic
            y = (y0 - dY) * ic
        return x * fx + cx, y * fy + cy


def undistort(K, D, u, v, iterations=5):
    """(u', v') float32 of float32 pixel coordinates: ugsm_undistort_points."""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    with np.errstate(all="ignore"):
        uo, vo = undistort64(K, D, u.astype(F64), v.astype(F64), iterations)
        return uo.astype(F32), vo.astype(F32)


def distort64(K, D, u, v):
    """The forward model: ideal pixel coordinates (float64) -> the distorted ones (float64)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = _cam(K, D)
    x, y = (np.asarray(u, F64) - cx) / fx, (np.asarray(v, F64) - cy) / fy
    r2 = x * x + y * y
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return xd * fx + cx, yd * fy + cy


def sq_d(v):
    v = v.astype(F64)
    return v * v


def tri_point(x1, y1, x2, y2, P1, P2):
    """X, Y, Z (float32 arrays) of float32 arrays x1, y1, x2, y2 of one shape."""
    x1, y1, x2, y2 = (np.asarray(q, F32) for q in (x1, y1, x2, y2))
    shape = np.broadcast_shapes(x1.shape, y1.shape, x2.shape, y2.shape)
    x1, y1, x2, y2 = (np.broadcast_to(q, shape) for q in (x1, y1, x2, y2))
    P1, P2 = np.asarray(P1, F64).reshape(12), np.asarray(P2, F64).reshape(12)
    two = np.full(shape, 2.0, F64)

    def const(v):
        return np.full(shape, F32(v), F32)

    with np.errstate(all="ignore"):
        a = const(P1[0])
        b = (P1[2] - x1.astype(F64)).astype(F32)
        c = const(P1[5])
        d = (P1[6] - y1.astype(F64)).astype(F32)
        e = (P2[0] - x2.astype(F64) * P2[8]).astype(F32)
        f = (P2[1] - x2.astype(F64) * P2[9]).astype(F32)
        g = (P2[2] - x2.astype(F64) * P2[10]).astype(F32)
        h = (P2[4] - y2.astype(F64) * P2[8]).astype(F32)
        i = (P2[5] - y2.astype(F64) * P2[9]).astype(F32)
        j = (P2[6] - y2.astype(F64) * P2[10]).astype(F32)
        x = (x2.astype(F64) * P2[11] - P2[3]).astype(F32)
        y = (y2.astype(F64) * P2[11] - P2[7]).astype(F32)
        for q in (a, b, c, d, e, f, g, h, i, j, x, y):
            assert q.dtype == F32
        XUp = ((d*f*h - c*g*h - d*e*i + c*e*j)*(-(d*i*x) + c*j*x + d*f*y - c*g*y) +
               sq_d(b)*((f*h - e*i)*(-(i*x) + f*y) + sq_d(c)*(e*x + h*y)) +
               a*b*((-(g*i) + f*j)*(i*x - f*y) + c*d*(f*x + i*y) - sq_d(c)*(g*x + j*y)))
        YUp = ((sq_d(b)*(f*h - e*i) + d*(d*f*h - c*g*h - d*e*i + c*e*j))*(h*x - e*y) +
               a*b*((c*d*e + g*h*i - two*f*h*j + e*i*j)*x + (c*d*h + f*g*h - two*e*g*i + e*f*j)*y) +
               sq_d(a)*((g*i - f*j)*(-(j*x) + g*y) + sq_d(d)*(f*x + i*y) - c*d*(g*x + j*y)))
        ZUp = (c*(-(d*f*h) + c*g*h + d*e*i - c*e*j)*(h*x - e*y) - a*b*((f*h - e*i)*(-(i*x) + f*y) +
               sq_d(c)*(e*x + h*y)) + sq_d(a)*((g*i - f*j)*(i*x - f*y) - c*d*(f*x + i*y) +
               sq_d(c)*(g*x + j*y)))
        divisor = (sq_d(b)*(sq_d(c)*(sq_d(e) + sq_d(h)) + sq_d(f*h - e*i)) +
                   sq_d(d*f*h - c*g*h - d*e*i + c*e*j) - two*a*b*(-(c*d*(e*f + h*i)) +
                   (f*h - e*i)*(-(g*i) + f*j) + sq_d(c)*(e*g + h*j)) + sq_d(a)*
                   (sq_d(d)*(sq_d(f) + sq_d(i)) + sq_d(g*i - f*j) - two*c*d*(f*g + i*j) +
                   sq_d(c)*(sq_d(g) + sq_d(j))))
        for q in (XUp, YUp, ZUp, divisor):
            assert q.dtype == F64
        XUp, YUp, ZUp, divisor = (q.astype(F32) for q in (XUp, YUp, ZUp, divisor))
        return np.stack([XUp / divisor, YUp / divisor, ZUp / divisor])


def tri_lens(x1, y1, x2, y2, P1, P2, lens=None):
    """tri_point of the two positions, each undistorted by its own camera where there is a lens."""
    if lens is not None:
        K1, D1, K2, D2, it = lens
        x1, y1 = undistort(K1, D1, x1, y1, it)
        x2, y2 = undistort(K2, D2, x2, y2, it)
    return tri_point(x1, y1, x2, y2, P1, P2)


def triangulate(dx, dy, P1, P2, lens=None):
    """ugsm_triangulate: (H, W) float32 disparities -> (3, H, W)."""
    dx, dy = np.asarray(dx, F32), np.asarray(dy, F32)
    H, W = dx.shape
    xx = np.broadcast_to(np.arange(W, dtype=F32)[None, :], (H, W))
    yy = np.broadcast_to(np.arange(H, dtype=F32)[:, None], (H, W))
    with np.errstate(all="ignore"):
        x2, y2 = xx + dx, yy + dy
    return tri_lens(xx, yy, x2, y2, P1, P2, lens)


def triangulate_fovea(stackx, stacky, level, left, upper, scale, P1, P2, lens=None):
    """ugsm_triangulate_fovea: level `level` of (F, fovH, fovW) stacks (finite, inside the range of int) -> (3, fovH, fovW).  The mapping
    first -- x1 = (float)left + (float)ii * scale, the right position from the TRUNCATED ii + dx --, then the lens."""
    sx, sy = np.asarray(stackx[level], F32), np.asarray(stacky[level], F32)
    fh, fw = sx.shape
    sc = F32(scale)
    ii = np.broadcast_to(np.arange(fw, dtype=F32)[None, :], (fh, fw))
    jj = np.broadcast_to(np.arange(fh, dtype=F32)[:, None], (fh, fw))
    x1 = F32(left) + ii * sc
    y1 = F32(upper) + jj * sc
    tx = np.trunc(ii + sx).astype(np.int32).astype(F32)
    ty = np.trunc(jj + sy).astype(np.int32).astype(F32)
    x2 = F32(left) + tx * sc
    y2 = F32(upper) + ty * sc
    for q in (x1, y1, x2, y2):
        assert q.dtype == F32
    return tri_lens(x1, y1, x2, y2, P1, P2, lens)


class LensOracle:
    """What tests/cloud_np.py, resize_np.py, depth_np.py and stack_cloud_np.py take as `orc`, with the planes of this module under `lens`
    (None: no lens): their records, resized maps, depth images and coverage rule then state the calls under a lens with nothing restated twice."""

    def __init__(self, lens=None):
        self.lens = lens

    def triangulate(self, dx, dy, P1, P2):
        return triangulate(dx, dy, P1, P2, self.lens)

    def triangulate_fovea(self, stackx, stacky, level, left, upper, scale, P1, P2):
        return triangulate_fovea(stackx, stacky, level, left, upper, scale, P1, P2, self.lens)
