"""CPU restatement of the depth image (ugsm_depth_image / ugsm_depth_image_fovea / ugsm_match_full_depth; include/ugsm.h) for the tests.

Z is the oracle's: orc.triangulate / orc.triangulate_fovea's third plane, and for a factor below 1 resize_np.resize_cubic of it, which already
pins the resized clouds.  What this file states is the REP 118 rule on top of it, every step an explicit float32 operation:
  valid  Z finite, z_min <= Z <= z_max, and (no confidence plane, or conf >= min_conf: a NaN confidence fails);
  32F    m = Z * unit where valid, else the quiet NaN 0x7FC00000;
  16U    u = (m * 1000.0f) + 0.5f; valid only with 1.0f <= u < 65536.0f; (uint16)u truncated where valid, else 0.
The confidence of pixel (ii, jj) of a resized image is conf(xx, yy), xx = (int)((float)ii / f), yy = (int)((float)jj / f).
"""
import numpy as np

import resize_np as rn

F32 = np.float32
FMT_32F, FMT_16U = 0, 1
QNAN = np.uint32(0x7FC00000)


def convert(Z, fmt=FMT_32F, unit=1.0, conf=None, min_conf=-np.inf, z_min=-np.inf, z_max=np.inf):
    """-> (image, valid mask) of a float32 Z map (and the confidence of each of its pixels)."""
    Z = np.asarray(Z, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(Z) & (Z >= F32(z_min)) & (Z <= F32(z_max))
        if conf is not None:
            valid &= np.asarray(conf, F32) >= F32(min_conf)          # (False for a NaN confidence)
        m = Z * F32(unit)
        assert m.dtype == F32
        if fmt == FMT_32F:
            img = np.where(valid, m.view(np.uint32), QNAN).astype(np.uint32).view(F32)
            return img, valid
        u = (m * F32(1000.0)) + F32(0.5)
        assert u.dtype == F32
        valid &= (u >= F32(1.0)) & (u < F32(65536.0))
        img = np.where(valid, u, F32(0)).astype(np.uint16)            # (truncation; u is in [1, 65536) wherever it is kept)
    return img, valid


def depth_of_z(z, conf=None, factor=1.0, **kw):
    """The image of a (ph, pw) Z plane: the plane itself at factor 1, else its cubic resize with the confidence read at (xx, yy)."""
    z = np.asarray(z, F32)
    ph, pw = z.shape
    if F32(factor) == F32(1.0):
        return convert(z, conf=conf, **kw)
    dw, dh = rn.resized_size(pw, ph, factor)
    c = None if conf is None else np.asarray(conf, F32)[np.ix_(rn.sample_at(ph, factor), rn.sample_at(pw, factor))]
    return convert(rn.resize_cubic(z, dw, dh), conf=c, **kw)


def depth_image(orc, dx, dy, P1, P2, conf=None, **kw):
    """ugsm_depth_image: dx, dy, conf (H, W) float32 planes -> (image, valid mask)."""
    return depth_of_z(orc.triangulate(dx, dy, P1, P2)[2], conf=conf, **kw)


def depth_image_fovea(orc, stackx, stacky, level, left, upper, scale, P1, P2, stackc=None, **kw):
    """ugsm_depth_image_fovea of one level: (F, fovH, fovW) stacks and the level's mapping -> (image, valid mask)."""
    z = orc.triangulate_fovea(stackx, stacky, level, left, upper, scale, P1, P2)[2]
    return depth_of_z(z, conf=None if stackc is None else stackc[level], **kw)


def image_bits(a):
    """The image's elements as unsigned integers: float32 by its bits (so that the NaN's payload counts), uint16 as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def assert_image_equal(got, exp, what=""):
    """Bit for bit, the NaN's payload included."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype}{got.shape} vs {exp.dtype}{exp.shape}"
    g, e = image_bits(got), image_bits(exp)
    if not (g == e).all():
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} pixels differ; first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} "
                             f"(0x{int(g[tuple(bad[0])]):x}) vs {exp[tuple(bad[0])]!r} (0x{int(e[tuple(bad[0])]):x})")


def assert_both_branches(valid, what=""):
    """A condition on a test's inputs: by the restatement at least 25 % of the pixels valid and at least 5 % invalid, so that a kernel
    which stores all-invalid (or all-valid) cannot pass."""
    share = float(np.mean(valid))
    assert 0.25 <= share <= 0.95, f"{what}: {share:.3f} of the pixels valid; the case must exercise both branches"
