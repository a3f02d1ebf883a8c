"""ugsm_reconstruct_full_multi's contract (include/ugsm.h) in NumPy, for the tests.

hierarchicalDisparity over the stacks of n windows of one pair: start from row block F-1 of stack 0 (the whole frame at level F-1, the same in
every stack); for level = F-1 .. 1 upsample to level-1 -- dst[y][x] = s * src[tex((y + .5f) / s)][tex((x + .5f) / s)], s = (float)1.41421356,
tex = floor then clamp, every channel scaled -- and paste level-1 of every stack at its window's origin at that level.  Windows are pasted
in ascending order, so where several hold a pixel the highest index wins.  float32 throughout; the products are np.float32(1.41421356) * v.
The window origins come from oracle.fovea_geometry.
"""
import numpy as np

S = np.float32(1.41421356)


def tex(n_dst, n_src):
    """The source index of every destination index 0 .. n_dst - 1: floor(((float)i + 0.5f) / s), clamped to the source."""
    c = (np.arange(n_dst, dtype=np.float32) + np.float32(0.5)) / S
    assert c.dtype == np.float32
    return np.clip(np.floor(c), 0, n_src - 1).astype(np.int64)


def reconstruct_multi(orc, stacks, W, H, levels, offsets):
    """stacks: n arrays (3, F, fovH, fovW) float32; offsets: n (off_x, off_y).  Returns (3, H, W) float32."""
    assert len(stacks) == len(offsets) >= 1
    F = stacks[0].shape[1]
    w, h = orc.level_dims(W, H, levels)
    geo = [orc.fovea_geometry(W, H, levels, F, int(ox), int(oy)) for ox, oy in offsets]
    fw, fh = geo[0][0], geo[0][1]
    cur = np.array(stacks[0][:, F - 1], np.float32)
    assert cur.shape == (3, h[F - 1], w[F - 1])
    for level in range(F - 1, 0, -1):
        sy, sx = tex(h[level - 1], h[level]), tex(w[level - 1], w[level])
        with np.errstate(invalid="ignore", over="ignore"):
            nxt = S * cur[:, sy[:, None], sx[None, :]]
        assert nxt.dtype == np.float32
        for k, g in enumerate(geo):
            ox, oy = g[2][level - 1], g[3][level - 1]
            nxt[:, oy:oy + fh, ox:ox + fw] = stacks[k][:, level - 1]
        cur = nxt
    assert cur.shape == (3, H, W)
    return cur


def random_stack(rng, F, fh, fw, specials=200):
    """A stack of finite values with NaN, +inf and -inf scattered through it."""
    st = rng.standard_normal((3, F, fh, fw)).astype(np.float32) * np.float32(7.0)
    flat = st.reshape(-1)
    at = rng.integers(0, flat.size, specials)
    flat[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), specials)
    return st
