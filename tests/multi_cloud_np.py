"""CPU restatement of the merged cloud of several fovea windows of one pair (ugsm_point_cloud_fovea_multi) for the tests, on
stack_cloud_np's functions.

  - entries: level-major -- entry k * n + j is level k < F-1 of window j, the last entry (F-1) * n is the whole-frame level F-1 of stack 0;
  - left_out: the rule across windows in float32.  Pixel (ii, jj) of entry (j, k) lies at x1 = (float)left[j][k] + (float)ii * scale_k
    (y1 alike); inside(i, m) says that [x1, x1 + scale_k) x [y1, y1 + scale_k) lies wholly inside level m's window of stack i, every
    operation rounded to binary32 on its own.  The pixel is left out when (a) k >= 1 and inside(i, k-1) for some window i, or
    (b) k <= F-2 and inside(i, k) for some i > j;
  - fovea_multi_cloud_points: the dense size and the sizes of the entries;
  - cloud_fovea_multi: the concatenation over the entries of cloud_np.cloud_fovea's dense records without the left-out ones, then the
    compaction filter, with stack_cloud_np's `undefined` provision for NaN / inf disparities (one record array per ENTRY here).
"""
import numpy as np

import cloud_np as cn
import stack_cloud_np as sn


def entries(F, n):
    """-> [(window j, level k)] in the cloud's order."""
    return [(j, k) for k in range(F - 1) for j in range(n)] + [(0, F - 1)]


def inside_1d(n, m, sc, m_other, sc_other):
    """Which of the n pixels at x1 = (float)m + (float)i * sc lie wholly inside [m_other, m_other + n * sc_other): the coverage rule
    along one axis (stack_cloud_np.covered_1d) against any window."""
    return sn.covered_1d(n, m, sc, m_other, sc_other)


def left_out(W, H, F, offsets, j, k):
    """-> (fovH, fovW) booleans: the pixels of level k of window j that the merged cloud leaves out."""
    fw, fh = sn.fovea_dims(W, H, F)
    l, u, sc = sn.level_mapping(W, H, F, k, offsets[j])
    out = np.zeros((fh, fw), bool)

    def add(i, m):
        lo, uo, so = sn.level_mapping(W, H, F, m, offsets[i])
        out[...] |= np.outer(inside_1d(fh, u, sc, uo, so), inside_1d(fw, l, sc, lo, so))
    if k >= 1:                                   # (a) a finer level of any window covers it
        for i in range(len(offsets)):
            add(i, k - 1)
    if k <= F - 2:                               # (b) the same level of a higher-numbered window holds it
        for i in range(j + 1, len(offsets)):
            add(i, k)
    return out


def fovea_multi_cloud_points(W, H, F, offsets, s=1):
    """-> (dense points of the merged cloud, the list per entry)."""
    per = [int((~left_out(W, H, F, offsets, j, k)[::s, ::s]).sum()) for j, k in entries(F, len(offsets))]
    return sum(per), per


def cloud_fovea_multi(orc, stacks, rgb, offsets, P1, P2, s=1, fmt=cn.PCL32, compact=False, min_conf=-np.inf, z_min=-np.inf,
                      z_max=np.inf, use_conf=True, undefined=None):
    """ugsm_point_cloud_fovea_multi: stacks = n arrays (3, F, fovH, fovW) (dx, dy, conf), rgb the (H, W, 3) left image ->
    (records, the number of records per entry).  use_conf: whether the confidence planes enter the compaction.  undefined: per
    entry, the dense records (same sampling and format) ugsm_point_cloud_fovea wrote, read only where the reference's integer
    conversion is undefined (stack_cloud_np's note)."""
    n = len(stacks)
    _, F, fh, fw = stacks[0].shape
    H, W, _ = rgb.shape
    item = cn.DTYPES[fmt].itemsize
    parts, per = [], []
    for e, (j, k) in enumerate(entries(F, n)):
        sx, sy, sc = stacks[j][0], stacks[j][1], stacks[j][2]
        left, upper, scale = sn.level_mapping(W, H, F, k, offsets[j])
        dense = cn.cloud_fovea(orc, sx, sy, k, left, upper, scale, rgb, P1, P2, s=s, fmt=fmt)
        undef = sn.undefined_conversion(sx, sy, k, s)
        if undef.any():
            if undefined is None:
                raise ValueError(f"entry {e}: {int(undef.sum())} pixels whose integer conversion the reference leaves undefined")
            assert undefined[e].dtype.itemsize == dense.dtype.itemsize and undefined[e].shape == dense.shape
            for name in ("x", "y", "z"):
                dense[name][undef] = undefined[e][name][undef]
        keep = ~cn.column_major(left_out(W, H, F, offsets, j, k), s)
        if compact:
            with np.errstate(invalid="ignore"):
                keep &= (np.isfinite(dense["x"]) & np.isfinite(dense["y"]) & np.isfinite(dense["z"]) & (dense["z"] >= np.float32(z_min)) &
                         (dense["z"] <= np.float32(z_max)))
                if use_conf:
                    keep &= cn.column_major(np.asarray(sc[k], np.float32), s) >= np.float32(min_conf)
        parts.append(np.ascontiguousarray(dense.view(np.uint8).reshape(-1, item)[keep]))
        per.append(int(keep.sum()))
    return np.concatenate(parts).reshape(-1).view(cn.DTYPES[fmt]), per
