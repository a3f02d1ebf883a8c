"""The seeded (warm) foveated call in numpy and oracle stages (test infrastructure), written from the definition in include/ugsm.h and not from
the kernel.  Stacks are (3, F, fovH, fovW) arrays: plane, row block, row, column -- the layout of a d_stack buffer.

    start_fields(orc, prior, W, H, levels, poff, off, s)       the definition: reconstruct -> restrict -> crop, {k: (3, fovH, fovW)} for k = s .. F-1
    start_fields_field(orc, field, W, H, levels, F, off, s)    the same from a full-resolution field: restrict -> crop
    pointwise(orc, prior, W, H, levels, poff, off, s)          a second, independent statement: the recursion per target pixel
    descend(orc, pl, pr, fields, W, H, levels, F, off, s)      the wanted stack: the starting fields above s, the matched levels s .. 0
    warm_oracle(orc, L, R, prior, levels, poff, off, s)        the stack ugsm_submit_foveated_warm must write, bit for bit
    special_stack(F, fh, fw, seed)                             a prior stack full of NaN, infinities, huge values, denormals and -0.0
"""
import numpy as np

import seeded_np as sn

S32 = np.float32(1.41421356)       # k_upsample_paste's `s`
HALF = np.float32(0.5)


def special_stack(F_, fh, fw, seed):
    """A prior stack with NaN, +-inf, +-3e38, denormals and -0.0 scattered over every plane and row block."""
    rng = np.random.default_rng(seed)
    st = rng.normal(0.0, 40.0, (3, F_, fh, fw)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 3e38, -3e38, 1e-44, -1e-45, 1.1754942e-38, 5e-39, 0.0], np.float32)
    flat = st.reshape(3 * F_, -1)
    for p in range(3 * F_):
        at = rng.integers(0, fh * fw, max(fh * fw // 5, 1))
        flat[p][at] = special[rng.integers(0, len(special), len(at))]
    return st


def origins(orc, W, H, levels, F, off):
    """(fw, fh, ox, oy, cx, cy) with the origin of level F-1 -- the whole level -- appended as 0."""
    fw, fh, ox, oy, cx, cy = orc.fovea_geometry(W, H, levels, F, off[0], off[1])
    return fw, fh, list(ox[:F - 1]) + [0], list(oy[:F - 1]) + [0], cx, cy


def _crops(orc, P, W, H, levels, F, off, s):
    lw, lh = orc.level_dims(W, H, levels)
    fw, fh, ox, oy, _, _ = origins(orc, W, H, levels, F, off)
    out = {}
    for k in range(s, F):
        r = sn.restrict_np(P, k, lw[k], lh[k])
        out[k] = np.ascontiguousarray(r[:, oy[k]:oy[k] + fh, ox[k]:ox[k] + fw])
        assert out[k].shape == (3, fh, fw), (k, out[k].shape)
    return out


def start_fields(orc, prior, W, H, levels, poff, off, s):
    prior = np.ascontiguousarray(prior, np.float32)
    P = orc.reconstruct_full(prior, W, H, levels, poff[0], poff[1])
    return _crops(orc, P, W, H, levels, prior.shape[1], off, s)


def start_fields_field(orc, field, W, H, levels, F, off, s):
    return _crops(orc, np.ascontiguousarray(field, np.float32), W, H, levels, F, off, s)


def pointwise(orc, prior, W, H, levels, poff, off, s):
    """Per target pixel: the level-0 site, V_0 by the recursion (V_l is row block l where the site lies inside the prior's window of level l,
    else S32 * V_{l+1} at tex_index((c + .5f) / S32)), the multiplications coarse to fine, then the restriction's value transform."""
    prior = np.ascontiguousarray(prior, np.float32)
    F = prior.shape[1]
    lw, lh = orc.level_dims(W, H, levels)
    fw, fh, nox, noy, _, _ = origins(orc, W, H, levels, F, off)
    _, _, pox, poy, _, _ = origins(orc, W, H, levels, F, poff)
    out = {}
    for k in range(s, F):
        sx = sn.sites_closed(lw[k], k, W)[nox[k]:nox[k] + fw]
        sy = sn.sites_closed(lh[k], k, H)[noy[k]:noy[k] + fh]
        x, y = np.meshgrid(sx, sy)                       # (fh, fw) level-0 sites
        val = np.zeros((3, fh, fw), np.float32)
        depth = np.full((fh, fw), -1, np.int64)
        for l in range(F):
            if l < F - 1:
                fx, fy = x - pox[l], y - poy[l]
                inside = (fx >= 0) & (fx < fw) & (fy >= 0) & (fy < fh)
            else:
                fx, fy, inside = x, y, np.ones((fh, fw), bool)
            take = inside & (depth < 0)
            val[:, take] = prior[:, l][:, fy[take], fx[take]]
            depth[take] = l
            if l < F - 1:
                x = sn.tex_index((x.astype(np.float32) + HALF) / S32, lw[l + 1])
                y = sn.tex_index((y.astype(np.float32) + HALF) / S32, lh[l + 1])
        with np.errstate(all="ignore"):
            for j in range(F - 1):                       # one multiplication per level descended, each rounded to binary32
                val = np.where(depth > j, S32 * val, val).astype(np.float32)
            h = k // 2
            for p in (0, 1):
                v = val[p]
                if k % 2:
                    v = (v.astype(np.float64) / sn.SCALE).astype(np.float32)
                if h:
                    v = v * np.float32(2.0 ** -h)
                val[p] = v
        out[k] = val
    return out


def descend(orc, pl, pr, fields, W, H, levels, F, off, s):
    """fields: {k: starting field} for k = s .. F-1.  pl, pr: the pyramids' levels (at least 0 .. s)."""
    fw, fh, ox, oy, cx, cy = origins(orc, W, H, levels, F, off)
    stack = np.empty((3, F, fh, fw), np.float32)
    for k in range(s + 1, F):
        stack[:, k] = fields[k]
    wup, hup = pl[F - 2].shape[2], pl[F - 2].shape[1]
    cur = fields[s]
    for i in range(s, -1, -1):
        if i < s:
            cur = orc.seed_fovea(cur, wup, hup, cx[i], cy[i])
        L3 = np.ascontiguousarray(pl[i][:, oy[i]:oy[i] + fh, ox[i]:ox[i] + fw])
        R3 = np.ascontiguousarray(pr[i][:, oy[i]:oy[i] + fh, ox[i]:ox[i] + fw])
        cur, _ = orc.iterate_level(L3, R3, cur, orc.iterations_for_level(i), orc.smooth_passes_for_level(i), False)
        stack[:, i] = cur
    return stack


def warm_oracle(orc, L, R, prior, levels, poff, off, s, pyr=None, field=False, F=None):
    """pyr: (pl, pr) of seeded_np.pyramids() where the caller holds them already.  field: `prior` is a full-resolution field (F then given)."""
    pl, pr = pyr if pyr is not None else sn.pyramids(orc, L, R, levels)
    H, W = pl[0].shape[1], pl[0].shape[2]
    if field:
        fields = start_fields_field(orc, prior, W, H, levels, F, off, s)
    else:
        F = np.asarray(prior).shape[1]
        fields = start_fields(orc, prior, W, H, levels, poff, off, s)
    return descend(orc, pl, pr, fields, W, H, levels, F, off, s)
