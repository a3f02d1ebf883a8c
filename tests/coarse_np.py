"""The full-mode call in two halves in numpy and oracle stages (test infrastructure): the prolongation as include/ugsm.h defines it, written
from that definition level by level and not from the kernel, and the two halves composed of the CPU oracle's stages.

    prolong_np(state3, dims)                          the (3, H, W) field of a field of level e = len(dims[0]) - 1; dims = (w[0 .. e], h[0 .. e])
    coarse_oracle(orc, L, R, e, levels)               the field ugsm_submit_full_coarse must write to d_state, bit for bit
    fine_oracle(orc, L, R, state3, e, levels)         the field ugsm_submit_full_fine must write from a state of level e
"""
import numpy as np

import seeded_np as sn

SF = np.float32(1 / sn.SCALE)   # subsampleDisp's sf = (float)(1 / SCALE), MatchLib.cu:372-401


def prolong_step(src3, w, h):
    """One step of the definition: P_l (3, h, w) from P_l+1 = src3."""
    src3 = np.ascontiguousarray(src3, np.float32)
    _, hs, ws = src3.shape
    sx = sn.tex_index((np.arange(w, dtype=np.int64).astype(np.float32) + sn.HALF) * SF, ws)
    sy = sn.tex_index((np.arange(h, dtype=np.int64).astype(np.float32) + sn.HALF) * SF, hs)
    with np.errstate(all="ignore"):
        return (sn.SCALE * src3[:, sy][:, :, sx].astype(np.float64)).astype(np.float32)


def prolong_np(state3, dims):
    w, h = dims
    e = len(w) - 1
    p = np.ascontiguousarray(state3, np.float32)
    assert p.shape == (3, h[e], w[e]), (p.shape, e)
    for l in range(e - 1, -1, -1):
        p = prolong_step(p, w[l], h[l])
    return p.copy()


def clamp_binds(n_fine, n_coarse):
    """Whether tex's clamp to n_coarse - 1 changes a site of the step from a level of n_fine columns to one of n_coarse."""
    f = np.floor((np.arange(n_fine, dtype=np.int64).astype(np.float32) + sn.HALF) * SF)
    return bool(f.max() > n_coarse - 1)


def coarse_oracle(orc, L, R, e, levels, pyr=None):
    """matchlevel on the levels top .. e from the zero seed, the top level with its exception, subsampleDisp between them: level e's field."""
    pl, pr = pyr if pyr is not None else sn.pyramids(orc, L, R, levels)
    top = levels - 1
    d = np.zeros_like(pl[top])
    for i in range(top, e - 1, -1):
        d, _ = orc.iterate_level(pl[i], pr[i], d, orc.iterations_for_level(i), orc.smooth_passes_for_level(i), i == top)
        if i > e:
            d = orc.seed(d, pl[i - 1].shape[2], pl[i - 1].shape[1])
    return d


def fine_oracle(orc, L, R, state3, e, levels, pyr=None):
    """subsampleDisp of the state to level e - 1, then matchlevel on the levels e - 1 .. 0; no level takes the top exception."""
    assert 1 <= e < levels
    pl, pr = pyr if pyr is not None else sn.pyramids(orc, L, R, levels)
    state3 = np.ascontiguousarray(state3, np.float32)
    assert state3.shape == pl[e].shape, (state3.shape, pl[e].shape)
    d = orc.seed(state3, pl[e - 1].shape[2], pl[e - 1].shape[1])
    return sn.descend(orc, pl, pr, d, e - 1, False)
