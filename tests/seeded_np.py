"""The seeded full-mode call in numpy and oracle stages (test infrastructure): the restriction as include/ugsm.h defines it, written from
that definition and not from the kernel, and the seeded match composed of the CPU oracle's stages.

    restrict_np(prior3, s, w, h)                      level s's starting field (3, h, w) from a full-resolution field (3, H, W)
    seeded_oracle(orc, L, R, prior3, s, levels)       the field ugsm_submit_full_seeded must write, bit for bit
    sites_closed(count, s, n) / sites_stepwise(...)   the sampling sites in closed form, and walked down the pyramid level by level
"""
import numpy as np

SCALE = 1.41421356          # MatchLib_common.h:15
SF1 = np.float32(SCALE)     # the pyramid's level-0 -> level-1 step: sf = (float)SCALE
SF2 = np.float32(2.0)       # ... and every level i -> i + 2 step: sf = 2.0f
HALF = np.float32(0.5)


def tex_index(coord, n):
    """clamp(floor(coord)) to 0 .. n - 1, NaN -> 0: the default-configured texture fetch (ugsm_device.hpp).  coord: float32 array."""
    assert coord.dtype == np.float32
    f = np.floor(coord)
    with np.errstate(invalid="ignore"):
        f = np.where(f >= 0, np.minimum(f, np.float32(n - 1)), np.float32(0))
    return f.astype(np.int64)


def sites_closed(count, s, n):
    """The level-0 column (row) each of the `count` columns (rows) of level s reads, of n: the closed form of the definition, with
    tex_index's clamp on the last step."""
    k, c = s // 2, np.arange(count, dtype=np.int64)
    if s % 2:
        c1 = ((c + 1) << k) - 1                                       # a level-1 column
        return tex_index((c1.astype(np.float32) + HALF) * SF1, n)
    if k == 0:
        return c
    c2 = ((c + 1) << (k - 1)) - 1                                     # a level-2 column; ((c + 1) << k) - 1 after the last step
    return tex_index((c2.astype(np.float32) + HALF) * SF2, n)


def sites_stepwise(s, dims):
    """The same by walking the pyramid's own sampling chain: level s -> s - 2 -> ... -> 0 or 1 (sf = 2.0f, clamped at every level's own
    size), then level 1 -> level 0 (sf = (float)SCALE).  dims: the sizes of the levels 0 .. s along this axis."""
    c, lev = np.arange(dims[s], dtype=np.int64), s
    while lev >= 2:
        c = tex_index((c.astype(np.float32) + HALF) * SF2, dims[lev - 2])
        lev -= 2
    if lev == 1:
        c = tex_index((c.astype(np.float32) + HALF) * SF1, dims[0])
    return c


def restrict_np(prior3, s, w, h):
    prior3 = np.ascontiguousarray(prior3, np.float32)
    _, H, W = prior3.shape
    k = s // 2
    sx, sy = sites_closed(w, s, W), sites_closed(h, s, H)
    out = prior3[:, sy][:, :, sx].copy()
    if s == 0:
        return out
    with np.errstate(all="ignore"):
        for p in (0, 1):
            v = out[p]
            if s % 2:
                v = (v.astype(np.float64) / SCALE).astype(np.float32)  # the partner of subsampleDisp's f32(SCALE * (double)v)
            if k:
                v = v * np.float32(2.0 ** -k)                          # binary32
            out[p] = v
    return out


def descend(orc, pl, pr, d, start, top_exception):
    """matchlevel on the levels start .. 0 from the field d of level start, subsampleDisp in between.  top_exception: level start is the
    pyramid's top level and takes the first-iteration exception (the cold call)."""
    for i in range(start, -1, -1):
        d, _ = orc.iterate_level(pl[i], pr[i], d, orc.iterations_for_level(i), orc.smooth_passes_for_level(i), top_exception and i == start)
        if i > 0:
            d = orc.seed(d, pl[i - 1].shape[2], pl[i - 1].shape[1])
    return d


def pyramids(orc, L, R, levels):
    return orc.pyramid(orc.rgb_to_planes(L), levels), orc.pyramid(orc.rgb_to_planes(R), levels)


def seeded_oracle(orc, L, R, prior3, s, levels, pyr=None):
    """pyr: (pl, pr) of pyramids() where the caller holds them already."""
    pl, pr = pyr if pyr is not None else pyramids(orc, L, R, levels)
    d = restrict_np(prior3, s, pl[s].shape[2], pl[s].shape[1])
    return descend(orc, pl, pr, d, s, False)


def cold_by_stages(orc, L, R, levels):
    """orc.match_full composed of the same stages: the zero seed at the top level, with its first-iteration exception."""
    pl, pr = pyramids(orc, L, R, levels)
    return descend(orc, pl, pr, np.zeros_like(pl[levels - 1]), levels - 1, True)
