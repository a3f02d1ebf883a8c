"""CPU restatement of the merged cloud of the whole fovea stack (ugsm_point_cloud_fovea_all) for the tests.

  - level_mapping: ugsm_fovea_level_mapping -- the reference's centred margins for any fovea_levels, moved by the window's clamped offset;
  - covered: the coverage rule in float32 -- pixel (ii, jj) of level k >= 1 is covered when its footprint [x1, x1 + scale_k) x
    [y1, y1 + scale_k) lies wholly inside level k-1's window, every operation rounded to binary32 on its own;
  - fovea_cloud_points: the dense size, per level (sampled columns) x (sampled rows) - (sampled covered columns) x (sampled covered rows);
  - cloud_fovea_all: the concatenation over the levels of cloud_np.cloud_fovea's dense records with the covered pixels removed, then
    the compaction filter (cloud_np.records').

Where the reference says nothing.  The foveated get3DPoint converts the right-image coordinate with (int)(ii + dx) and (int)(jj + dy).  C
leaves that conversion undefined for a NaN and for a value outside int's range (C11 6.3.1.4): the oracle, compiled for x86, yields INT_MIN
for all of them, the device's conversion saturates (NaN to 0, +inf to INT_MAX), and neither is "the" answer.  A stack the matcher produced
holds no such value; a random stack salted with NaN and inf does.  For exactly those pixels (undefined_conversion) cloud_fovea_all takes
X, Y, Z from the records ugsm_point_cloud_fovea wrote for the level (`undefined`), which is what the header defines the merged cloud's
record to be; every other pixel's X, Y, Z are the oracle's, and the colour, the coverage rule, the order, the compaction filter and the
counts are restated here for all of them.  Without `undefined`, a stack with such a pixel is refused rather than compared against noise.
"""
import numpy as np

import cloud_np as cn

K_SCALE = 1.41421356  # the pyramid's scale (a double), as the library's level sizes use it


def level_dims(W, H, n):
    w, h = [W], [H]
    for _ in range(n - 1):
        w.append(int(w[-1] / K_SCALE))
        h.append(int(h[-1] / K_SCALE))
    return w, h


def fovea_dims(W, H, F):
    w, h = level_dims(W, H, F)
    return w[F - 1], h[F - 1]


def scale_of(k):
    """powf((float)1.41421356237309504880, (float)k): the float32 nearest the double power of the float32 root."""
    return np.float32(float(np.float32(1.41421356237309504880)) ** int(k))


def level_mapping(W, H, F, k, off=(0, 0)):
    """-> (left_margin, upper_margin, scale) of level k of an F-level stack whose windows were moved by `off` (level-0 pixels)."""
    w, h = level_dims(W, H, F)

    def margin(d, o):
        f, e = d[F - 1], 0
        if k < F - 1:   # the window's clamped offset from the centre at level k
            cc = d[k] // 2 - f // 2
            e = min(max(cc + int(np.rint(o / K_SCALE ** k)), 0), d[k] - f) - cc
        return d[0] // 2 - d[F - 1 - k] // 2 + int(np.rint(e * K_SCALE ** k))
    return margin(w, off[0]), margin(h, off[1]), scale_of(k)


def covered_1d(n, m, sc, m_fine, sc_fine):
    """The rule along one axis: which of the n pixels at x1 = (float)m + (float)i * sc lie wholly inside [m_fine, m_fine + n * sc_fine)."""
    sc, sc_fine = np.float32(sc), np.float32(sc_fine)
    x1 = np.float32(m) + np.arange(n, dtype=np.float32) * sc
    hi = np.float32(m_fine) + np.float32(n) * sc_fine
    return (x1 >= np.float32(m_fine)) & (x1 + sc <= hi)


def covered(W, H, F, k, off=(0, 0)):
    """-> (covered columns (fovW,), covered rows (fovH,)) of level k, booleans; pixel (ii, jj) is covered when both are."""
    fw, fh = fovea_dims(W, H, F)
    if k == 0:
        return np.zeros(fw, bool), np.zeros(fh, bool)
    l, u, s = level_mapping(W, H, F, k, off)
    lf, uf, sf = level_mapping(W, H, F, k - 1, off)
    cols, rows = covered_1d(fw, l, s, lf, sf), covered_1d(fh, u, s, uf, sf)
    if not cols.any() or not rows.any():
        cols[:], rows[:] = False, False
    return cols, rows


def fovea_cloud_points(W, H, F, off=(0, 0), s=1):
    """-> (dense points of the merged cloud, the list per level)."""
    fw, fh = fovea_dims(W, H, F)
    per = []
    for k in range(F):
        cols, rows = covered(W, H, F, k, off)
        per.append(-(-fw // s) * -(-fh // s) - int(cols[::s].sum()) * int(rows[::s].sum()))
    return sum(per), per


def undefined_conversion(stackx, stacky, k, s=1):
    """The sampled pixels of level k, in the cloud's order, whose (int)(ii + dx) or (int)(jj + dy) C leaves undefined: the float32 sum
    is a NaN or its truncation does not fit an int."""
    _, fh, fw = stackx.shape
    with np.errstate(invalid="ignore"):
        vx = np.arange(fw, dtype=np.float32)[None, :] + np.asarray(stackx[k], np.float32)
        vy = np.arange(fh, dtype=np.float32)[:, None] + np.asarray(stacky[k], np.float32)
        ok = (vx >= np.float32(-2147483648.0)) & (vx < np.float32(2147483648.0)) & (vy >= np.float32(-2147483648.0)) & (vy < np.float32(2147483648.0))
    return cn.column_major(~ok, s)


def cloud_fovea_all(orc, stackx, stacky, rgb, off, P1, P2, stackc=None, s=1, fmt=cn.PCL32, compact=False, min_conf=-np.inf,
                    z_min=-np.inf, z_max=np.inf, undefined=None):
    """ugsm_point_cloud_fovea_all: (F, fovH, fovW) stacks, rgb the (H, W, 3) left image -> (records, the number of records per level).
    undefined: per level, the dense records (same sampling and format) ugsm_point_cloud_fovea wrote, read only where the reference's
    integer conversion is undefined (the module's note)."""
    F, fh, fw = stackx.shape
    H, W, _ = rgb.shape
    item = cn.DTYPES[fmt].itemsize
    parts, per = [], []
    for k in range(F):
        left, upper, scale = level_mapping(W, H, F, k, off)
        dense = cn.cloud_fovea(orc, stackx, stacky, k, left, upper, scale, rgb, P1, P2, s=s, fmt=fmt)
        undef = undefined_conversion(stackx, stacky, k, s)
        if undef.any():
            if undefined is None:
                raise ValueError(f"level {k}: {int(undef.sum())} pixels whose integer conversion the reference leaves undefined")
            assert undefined[k].dtype.itemsize == dense.dtype.itemsize and undefined[k].shape == dense.shape
            for name in ("x", "y", "z"):
                dense[name][undef] = undefined[k][name][undef]
        cols, rows = covered(W, H, F, k, off)
        keep = ~np.outer(cols[::s], rows[::s]).reshape(-1)   # (column outer, row inner: the cloud's order)
        if compact:
            with np.errstate(invalid="ignore"):
                keep &= (np.isfinite(dense["x"]) & np.isfinite(dense["y"]) & np.isfinite(dense["z"]) & (dense["z"] >= np.float32(z_min)) &
                         (dense["z"] <= np.float32(z_max)))
                if stackc is not None:
                    keep &= cn.column_major(np.asarray(stackc[k], np.float32), s) >= np.float32(min_conf)
        parts.append(np.ascontiguousarray(dense.view(np.uint8).reshape(-1, item)[keep]))
        per.append(int(keep.sum()))
    return np.concatenate(parts).reshape(-1).view(cn.DTYPES[fmt]), per
