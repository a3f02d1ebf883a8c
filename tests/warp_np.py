"""The warped right image and the photometric residual of a match (include/ugsm.h, "the warped right image ..."), restated in numpy --
test infrastructure, shared by tests/test_warp_host.py, tests/test_gpu_warp.py and tests/golden/make_warp_golden.py.

warp: the fetch of the reference's `warp` stage (MatchLib.cu:499-549) through the texture index of tests/golden/restate_np.py.
residual_sums: the four binary64 sums in the fixed order of row f-4, written out sequentially -- np.sum is pairwise and does not reproduce it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import restate_np as rn  # noqa: E402

F32, F64 = np.float32, np.float64
SHAPES = [(37, 29), (130, 75), (160, 120), (333, 217)]   # the fixture's (W, H)
WILD = (130, 75)                                          # ... and the one that carries a second, wild field
PAIR_SEED, FIELD_SEED = 9400, 9500                        # + the shape's index


def warp(src, dx, dy):
    """warp(src, dx, dy)[iy][ix] = src[tex(((float)iy + 0.5f) + dy)][tex(((float)ix + 0.5f) + dx)]; src (H, W) or (.., H, W)."""
    H, W = src.shape[-2:]
    with np.errstate(all="ignore"):
        cx = (np.arange(W, dtype=F32)[None, :] + F32(0.5)) + np.asarray(dx, F32)
        cy = (np.arange(H, dtype=F32)[:, None] + F32(0.5)) + np.asarray(dy, F32)
    return np.ascontiguousarray(src[..., rn.tex_idx(cy, H), rn.tex_idx(cx, W)])


def _ordered(v):
    """sum of v (.., n) over its last axis: lane l = i mod 64 adds its elements in order from 0.0, the 64 lane sums in lane order from 0.0"""
    n = v.shape[-1]
    lanes = np.zeros(v.shape[:-1] + (64,), F64)
    for i in range(n):
        lanes[..., i % 64] += v[..., i]
    out = np.zeros(v.shape[:-1], F64)
    for l in range(64):
        out = out + lanes[..., l]
    return out


def residual_sums(L3, Rw3, conf=None):
    """[S_0, S_1, S_2, C] as float64: t = fabsf(L_c - R'_c) in float, t = t * conf in float (conf None: 1.0f), summed in binary64 in the
    order of row f-4 -- within a row over x mod 64, the rows over y mod 64."""
    L3, Rw3 = np.asarray(L3, F32), np.asarray(Rw3, F32)
    c = np.ones(L3.shape[-2:], F32) if conf is None else np.asarray(conf, F32)
    with np.errstate(all="ignore"):
        t = np.abs(L3 - Rw3).astype(F32) * c[None]
        terms = np.concatenate([t.astype(F32), c[None]]).astype(F64)   # (4, H, W)
        return _ordered(_ordered(terms))


def residual(L3, Rw3, conf=None):
    """(float32(S_c / C) for the three channels, C)"""
    s = residual_sums(L3, Rw3, conf)
    with np.errstate(all="ignore"):
        return (s[:3] / s[3]).astype(F32), s[3]


def wild_field(W, H, seed):
    """seed_field's (dx, dy) with wild entries scattered in: NaN, +-inf, +-3e38, +-2^31, -0.5, denormals"""
    import ref_stages as rs
    d = rs.seed_field(W, H, seed)[:2].copy()
    vals = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -(2.0 ** 31), -0.5, 1e-40, -1e-40], F32)
    rng = np.random.Generator(np.random.PCG64(seed + 7))
    for k in range(2):
        at = rng.choice(W * H, 40 * len(vals), replace=False)
        d[k].reshape(-1)[at] = np.tile(vals, 40)
    d[0, 0, 0], d[1, 0, 0], d[0, -1, -1], d[1, -1, -1] = np.nan, np.inf, -np.inf, np.nan
    return d


def fixture_inputs(k):
    """The inputs of shape k of the fixture, from its seeds: (L, R) uint8 images, the (dx, dy, conf) field, the wild (dx, dy) or None."""
    import ref_stages as rs
    W, H = SHAPES[k]
    L, R = rs.pair(W, H, PAIR_SEED + k)
    d = rs.seed_field(W, H, FIELD_SEED + k)
    return L, R, d, (wild_field(W, H, FIELD_SEED + 50 + k) if (W, H) == WILD else None)


def planes(rgb):
    return np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(F32)
