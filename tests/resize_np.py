"""CPU restatement of the resized cloud (ugsm_point_cloud_resized[_fovea]; getPointCloud.cpp doReconstruction_resized, :724-800, and
doReconstructionFOV_resized, :802-884) for the tests.

The Z plane is resized with cv::resize(..., INTER_CUBIC) to dw x dh = (int)((float)pw * f) x (int)((float)ph * f).  On CV_32F that is
OpenCV's generic path (resizeGeneric_ with HResizeCubic / VResizeCubic), restated here in float32 with nothing promoted to float64 but
the tap positions, which OpenCV computes in double:
  - scale = 1. / ((double)dw / pw); fx = (float)((dx + 0.5) * scale - 0.5); sx = floor(fx); fx -= sx (float); rows the same with dy;
  - A = -0.75f: c0 = ((A*(x+1) - 5*A)*(x+1) + 8*A)*(x+1) - 4*A, c1 = ((A+2)*x - (A+3))*x*x + 1,
    c2 = ((A+2)*(1-x) - (A+3))*(1-x)*(1-x) + 1, c3 = 1.f - c0 - c1 - c2, all in float;
  - taps sx-1 .. sx+2, sy-1 .. sy+2, clamped to the plane (replicate border);
  - horizontal pass first, on every source row: S[sx-1]*c0 + S[sx]*c1 + S[sx+1]*c2 + S[sx+2]*c3 left to right; on the border columns
    (dx < xmin or dx >= xmax: xmin = 1 + the last dx with sx < 1, xmax = the first dx with sx + 2 >= pw) the sum starts from +0.0f;
  - vertical pass: ((R0*b0 + R1*b1) + R2*b2) + R3*b3; every product rounded on its own (no FMA); NaN and inf propagate;
  - cv::resize copies the plane when the size does not change (factor 1).
OpenCV builds that take IPP or an FMA-dispatched vertical pass can differ in the last bit; OpenCV is not a dependency, so the
restatement is not pinned against it.

Points: column ii outer, row jj inner; xx = (int)((float)ii / f), yy = (int)((float)jj / f) in float32; X, Y of the pixel (xx, yy), Z the
resized map's (ii, jj), the colour at (xx, yy) -- the foveated form reads it there too, in the full image (the reference's quirk), or at
the mapped pixel with colour_mapped; compaction tests X, Y, the resized Z and conf(xx, yy).
"""
import numpy as np

from cloud_np import assert_cloud_equal, colour_word, fovea_colour_at, records  # noqa: F401  (assert_cloud_equal: for the tests)

F32 = np.float32
A = F32(-0.75)


def resized_size(W, H, factor):
    """cv::Size(W * f, H * f): float32 products truncated to int."""
    f = F32(factor)
    return int(F32(W) * f), int(F32(H) * f)


def tap_table(n, m):
    """OpenCV's taps for a side resized from n to m: (s, coeffs (m, 4) float32, border (m,) bool)."""
    scale = 1.0 / (m / n)                                       # double, as resize.cpp
    fx = ((np.arange(m, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(fx).astype(np.int64)
    x = fx - s.astype(F32)
    one, x1, xm = F32(1), x + F32(1), F32(1) - x
    c0 = ((A * x1 - F32(5) * A) * x1 + F32(8) * A) * x1 - F32(4) * A
    c1 = ((A + F32(2)) * x - (A + F32(3))) * x * x + one
    c2 = ((A + F32(2)) * xm - (A + F32(3))) * xm * xm + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], axis=1).astype(F32)
    assert c.dtype == F32
    lo = np.nonzero(s < 1)[0]
    xmin = int(lo[-1]) + 1 if lo.size else 0
    hi = np.nonzero(s + 2 >= n)[0]
    xmax = int(hi[0]) if hi.size else m
    d = np.arange(m)
    return s, c, (d < xmin) | (d >= xmax)


def resize_cubic(plane, dw, dh):
    """cv::resize(plane, Size(dw, dh), 0, 0, INTER_CUBIC) of a float32 (ph, pw) plane, restated."""
    plane = np.asarray(plane, F32)
    ph, pw = plane.shape
    if (dw, dh) == (pw, ph):
        return plane.copy()
    sx, cx, border = tap_table(pw, dw)
    sy, cy, _ = tap_table(ph, dh)
    cols = np.clip(sx[:, None] + np.arange(-1, 3)[None, :], 0, pw - 1)          # (dw, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        taps = plane[:, cols]                                                    # (ph, dw, 4)
        prod = taps * cx[None, :, :]
        h = np.where(border[None, :], F32(0) + prod[..., 0], prod[..., 0])
        for k in range(1, 4):
            h = h + prod[..., k]
        rows = np.clip(sy[:, None] + np.arange(-1, 3)[None, :], 0, ph - 1)      # (dh, 4)
        v = h[rows[:, 0]] * cy[:, 0:1]
        for k in range(1, 4):
            v = v + h[rows[:, k]] * cy[:, k:k + 1]
    assert v.dtype == F32
    return v


def sample_at(n, factor):
    """xx = (int)((float)i / f) for i < (int)(n * f): float32 division, truncated."""
    m = int(F32(n) * F32(factor))
    return (np.arange(m, dtype=F32) / F32(factor)).astype(np.int64)


def _resized_records(xyz, word, conf, factor, **kw):
    ph, pw = xyz.shape[1:]
    dw, dh = resized_size(pw, ph, factor)
    xs, ys = sample_at(pw, factor), sample_at(ph, factor)
    sel = np.ix_(ys, xs)
    plane = np.stack([xyz[0][sel], xyz[1][sel], resize_cubic(xyz[2], dw, dh)])
    return records(plane, word[sel], conf=None if conf is None else conf[sel], **kw)


def resized_cloud(orc, dx, dy, rgb, P1, P2, factor, conf=None, **kw):
    """ugsm_point_cloud_resized: dx, dy, conf (H, W) float32 planes, rgb (H, W, 3) uint8."""
    return _resized_records(orc.triangulate(dx, dy, P1, P2), colour_word(rgb), conf, factor, **kw)


def resized_cloud_fovea(orc, stackx, stacky, src_level, left, upper, scale, rgb, P1, P2, factor, stackc=None, colour_mapped=0, **kw):
    """ugsm_point_cloud_resized_fovea: (F, fovH, fovW) stacks, level src_level; rgb the (H, W, 3) full-resolution left image."""
    _, fh, fw = stackx.shape
    H, W, _ = rgb.shape
    xyz = orc.triangulate_fovea(stackx, stacky, src_level, left, upper, scale, P1, P2)
    if colour_mapped:
        cx, cy, _ = fovea_colour_at(W, H, fw, fh, left, upper, scale)
    else:   # the unmapped pixel of the full image (clamped, as the device; inert while the fovea is no larger than the image)
        cx, cy = np.minimum(np.arange(fw), W - 1), np.minimum(np.arange(fh), H - 1)
    word = colour_word(rgb)[np.ix_(cy, cx)]
    conf = stackc[src_level] if stackc is not None else None
    return _resized_records(xyz, word, conf, factor, **kw)
