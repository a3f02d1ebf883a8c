"""CPU restatement of the coloured point cloud (ugsm_point_cloud / ugsm_point_cloud_fovea; getPointCloud.cpp doReconstructionRGB,
:675-722, and doReconstructionRGB_FOV, :615-673) for the tests.

X, Y, Z come from the oracle's triangulate / triangulate_fovea (get3DPoint); what this module adds is the rest of the contract:
  - order: column ii outer, row jj inner -- record (ci, cj) of the sampled grid is record ci * hc + cj;
  - sampling: pixel (ii, jj) is taken when ii % s == 0 and jj % s == 0;
  - colour word: byte0 << 16 | byte1 << 8 | byte2 of the rgb8 left image (R << 16 | G << 8 | B of the node's BGR8 copy), alpha 0;
    the foveated form reads it at ((int)x1, (int)y1), x1 = (float)left + (float)ii * scale, clamped to the image;
  - records: PCL32 = x, y, z, 1.0f, rgb word, 12 zero bytes; XYZRGB16 = x, y, z, rgb word;
  - compaction: keep finite X, Y, Z with z_min <= Z <= z_max and (with a confidence plane) conf >= min_conf, in dense order.
"""
import numpy as np

PCL32, XYZRGB16 = 0, 1
DT_PCL32 = np.dtype({"names": ["x", "y", "z", "w", "rgb"], "formats": [np.float32, np.float32, np.float32, np.float32, np.uint32],
                     "offsets": [0, 4, 8, 12, 16], "itemsize": 32})
DT_XYZRGB16 = np.dtype({"names": ["x", "y", "z", "rgb"], "formats": [np.float32, np.float32, np.float32, np.uint32],
                        "offsets": [0, 4, 8, 12], "itemsize": 16})
DTYPES = {PCL32: DT_PCL32, XYZRGB16: DT_XYZRGB16}


def cloud_points(W, H, s):
    return -(-W // s) * -(-H // s)


def colour_word(rgb):
    """(H, W, 3) uint8 -> (H, W) uint32: byte0 << 16 | byte1 << 8 | byte2."""
    rgb = rgb.astype(np.uint32)
    return (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]


def column_major(plane, s):
    """The sampled pixels of a (ph, pw) plane in the cloud's order: columns outer, rows inner."""
    return np.ascontiguousarray(plane[::s, ::s].T).reshape(-1)


def records(xyz, word, s=1, fmt=PCL32, conf=None, compact=False, min_conf=-np.inf, z_min=-np.inf, z_max=np.inf):
    """The cloud from X, Y, Z planes (3, ph, pw) and the colour word of each pixel (ph, pw): a structured array of DTYPES[fmt]."""
    X, Y, Z = (column_major(np.asarray(xyz[k], np.float32), s) for k in range(3))
    rgb = column_major(np.asarray(word, np.uint32), s)
    out = np.zeros(X.size, DTYPES[fmt])
    out["x"], out["y"], out["z"], out["rgb"] = X, Y, Z, rgb
    if fmt == PCL32:
        out["w"] = 1.0
    if compact:
        with np.errstate(invalid="ignore"):
            keep = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z >= np.float32(z_min)) & (Z <= np.float32(z_max))
            if conf is not None:
                keep &= column_major(np.asarray(conf, np.float32), s) >= np.float32(min_conf)
        # (selected through a byte view: indexing a structured array with padding does not carry the pad bytes)
        item = out.dtype.itemsize
        out = np.ascontiguousarray(out.view(np.uint8).reshape(-1, item)[keep]).view(out.dtype).reshape(-1)
    return out


def cloud(orc, dx, dy, rgb, P1, P2, conf=None, **kw):
    """ugsm_point_cloud: dx, dy, conf (H, W) float32 planes, rgb (H, W, 3) uint8."""
    return records(orc.triangulate(dx, dy, P1, P2), colour_word(rgb), conf=conf, **kw)


def fovea_colour_at(W, H, fw, fh, left, upper, scale):
    """The full-resolution pixel each fovea pixel takes its colour from -- ((int)mapXcoord(ii), (int)mapYcoord(jj)), float arithmetic
    as k_triangulate_fovea's x1 / y1 -- clamped to the image; and whether the clamp changed any of them."""
    sc = np.float32(scale)
    x1 = np.float32(left) + np.arange(fw, dtype=np.float32) * sc
    y1 = np.float32(upper) + np.arange(fh, dtype=np.float32) * sc
    cx, cy = np.trunc(x1).astype(np.int64), np.trunc(y1).astype(np.int64)
    fired = bool((cx < 0).any() or (cx > W - 1).any() or (cy < 0).any() or (cy > H - 1).any())
    return np.clip(cx, 0, W - 1), np.clip(cy, 0, H - 1), fired


def cloud_fovea(orc, stackx, stacky, src_level, left, upper, scale, rgb, P1, P2, stackc=None, **kw):
    """ugsm_point_cloud_fovea: (F, fovH, fovW) stacks, level src_level; rgb the (H, W, 3) full-resolution left image."""
    _, fh, fw = stackx.shape
    H, W, _ = rgb.shape
    xyz = orc.triangulate_fovea(stackx, stacky, src_level, left, upper, scale, P1, P2)
    cx, cy, _ = fovea_colour_at(W, H, fw, fh, left, upper, scale)
    word = colour_word(rgb)[np.ix_(cy, cx)]
    conf = stackc[src_level] if stackc is not None else None
    return records(xyz, word, conf=conf, **kw)


def assert_cloud_equal(got, exp, what=""):
    """Byte for byte, except that a NaN X, Y or Z equals any NaN (as conftest.assert_bit_equal)."""
    assert got.dtype.itemsize == exp.dtype.itemsize and got.shape == exp.shape, f"{what}: {got.shape} vs {exp.shape}"
    words = got.dtype.itemsize // 4
    g = np.ascontiguousarray(got).view(np.uint32).reshape(got.size, words)
    e = np.ascontiguousarray(exp).view(np.uint32).reshape(exp.size, words)
    same = g == e
    gf, ef = g[:, :3].view(np.float32), e[:, :3].view(np.float32)
    same[:, :3] |= np.isnan(gf) & np.isnan(ef)
    if not same.all():
        bad = np.argwhere(~same)
        r, w = bad[0]
        raise AssertionError(f"{what}: {len(np.unique(bad[:, 0]))} of {got.size} records differ; first record {r}, word {w}: "
                             f"{g[r].tolist()} vs {e[r].tolist()}")
